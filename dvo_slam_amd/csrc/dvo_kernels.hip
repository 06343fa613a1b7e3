// HIP kernels (gfx950 / CDNA4) of the dense RGB-D alignment hot path.
//
//  k_tick      one launch per Gauss-Newton tick.  blockIdx.y selects a WorkItem:
//              - residual pass  = computeResidualsSse + computeWeightsSse + computeScaleSse + Jacobians +
//                NormalEquationsLeastSquares::update fused (dense_tracking_impl.cpp:133-393,590-707,
//                dense_tracking.cpp:333-342,448-476, math_sse.cpp:82-178): one read of the reference planes, one
//                bilinear gather of the current planes, residuals spilled once (8 B/px) for the log-likelihood;
//              - log-likelihood pass = computeCompleteDataLogLikelihood (dense_tracking_impl.cpp:406-425).
//  k_finalize  second-pass block reduce: ordered combine of the per-block records (fp64), one block per job.
//  prep kernels: pyramid down-sampling, derivatives, gather layout, point selection (rgbd_image.cpp, point_selection.cpp).
//
// Numerics: the reference evaluates the warp/residual stage in round-toward-zero (MXCSR, dense_tracking_impl.cpp:165-167)
// and everything else in round-to-nearest.  The residual section below switches MODE.FP_ROUND the same way, is compiled
// without fp contraction, and forms 1/z as the exactly truncated quotient, so every residual and every validity decision
// is bit-identical to the CPU restatement in oracle/ (rcp_mode = EXACT).  Sums are accumulated per thread in fp32 (fma),
// reduced across a wave with DPP, across waves through LDS and across blocks in fp64 by k_finalize, in a fixed order
// (deterministic run to run).
//
// This file is compiled with -ffp-contract=off: every a*b+c that may fuse is written as __builtin_fmaf explicitly.
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <mutex>
#include <vector>

#include "dvo_launch_rules.h"
#include "dvo_types.h"

namespace dvo_amd {

// ------------------------------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------------------------------

// hwreg(HW_REG_MODE, offset 0, width 2) = single-precision rounding mode: 0 nearest-even, 3 toward zero
#define DVO_HWREG_MODE_FP32_ROUND (1 | (0 << 6) | ((2 - 1) << 11))
// Make a value opaque to the optimiser.  Every float that is live across a rounding-mode switch goes through this once
// before and once after the s_setreg, so no operation producing or consuming it can be scheduled on the wrong side.
#define DVO_OPAQUE(x) asm volatile("" : "+v"(x))
#ifndef DVO_KT_SGPR
#define DVO_KT_SGPR 1
#endif

__device__ __forceinline__ void round_toward_zero() { __builtin_amdgcn_s_setreg(DVO_HWREG_MODE_FP32_ROUND, 3); }
__device__ __forceinline__ void round_to_nearest() { __builtin_amdgcn_s_setreg(DVO_HWREG_MODE_FP32_ROUND, 0); }

// v_mul_legacy_f32: 0 * x = 0 for every x (NaN and infinity included); otherwise an ordinary IEEE multiply
__device__ __forceinline__ float mul_legacy(float a, float b) {
  float r;
  asm("v_mul_legacy_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ __forceinline__ float u2f(unsigned u) { return __builtin_bit_cast(float, u); }
__device__ __forceinline__ unsigned f2u(float f) { return __builtin_bit_cast(unsigned, f); }

// DPP move: returns 0 in lanes the row mask disables or whose source is invalid
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_read(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xF, true));
}

// Sum over the 64 lanes of a wave with DPP row operations; the total is valid in lane 63.
__device__ __forceinline__ float wave_sum_to_lane63(float v) {
  v += dpp_read<0xB1, 0xF>(v);   // quad_perm [1,0,3,2]
  v += dpp_read<0x4E, 0xF>(v);   // quad_perm [2,3,0,1]
  v += dpp_read<0x141, 0xF>(v);  // row_half_mirror
  v += dpp_read<0x140, 0xF>(v);  // row_mirror: every lane holds its row's sum
  v += dpp_read<0x142, 0xA>(v);  // row_bcast15 into rows 1 and 3
  v += dpp_read<0x143, 0xC>(v);  // row_bcast31 into rows 2 and 3
  return v;
}

__device__ __forceinline__ double wave_sum_double(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// Blocks b and b+8 share an XCD (round-robin dispatch); give each XCD one contiguous run of logical blocks so that
// neighbouring scan-order ranges (which gather overlapping rows of the current image) meet in the same 4 MiB L2.
// Bijective for any n_blocks; affects speed only.
__device__ __forceinline__ int xcd_contiguous_block(int b, int n_blocks) {
  const int q = n_blocks >> 3, r = n_blocks & 7;
  const int xcd = b & 7, pos = b >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
}

// trunc(1/z): the quotient rounded toward zero.  MUST run with MODE.FP_ROUND = toward zero (project_pixel_rtz does).
// r = v_rcp_f32(|z|) is within 1 ulp of rho = 1/|z|: r = rho (1 + d), |d| <= 2^-22.  One Newton step r' = r + r (1 - |z| r),
// its residual e = 1 - |z| r exact in one fma (|z| r is within 2^-22 of 1) and the step itself one fma ROUNDED TOWARD ZERO,
// evaluates V = rho (1 - d^2): below rho by at most rho 2^-44, far less than the spacing of floats there.  So r' = floor(V) is
// the truncated quotient T or its lower neighbour, and the sign of the exact residual 1 - |z| nextup(r') (again one fma: a
// non-zero value never rounds across zero) tells which.  NaN goes through as NaN (every compare is false, every candidate a
// NaN): an unselected reference pixel -- depth NaN by construction, i.e. most lanes of most steps -- costs nothing extra.
// Zero, denormal, huge and infinite |z| (never a pixel that ends up in bounds with a sane pose, but the result must still be
// the division's) take the IEEE division; until round 3 NaN lanes took it too, on three of four wave steps.
__device__ __forceinline__ float rcp_toward_zero(float z) {
  const float az = __builtin_fabsf(z);
  if (__builtin_expect(az < 1.1754944e-38f || az > 8.5070592e+37f, 0)) return 1.0f / z;  // (ordered compares: false for NaN)
  const float r = __builtin_amdgcn_rcpf(az);
  const float e = __builtin_fmaf(-az, r, 1.0f);
  const unsigned lo = f2u(__builtin_fmaf(e, r, r));  // T or T - 1 ulp (toward-zero rounding)
  const unsigned up = lo + 1u;
  const bool up_fits = __builtin_fmaf(-az, u2f(up), 1.0f) >= 0.0f;  // nextup(r') <= 1/|z|
  return __builtin_copysignf(u2f(up_fits ? up : lo), z);
}

// The host's _mm_rcp_ps (opt-in, dvo_amd_set_reciprocal_mode): rcpps(x) = rcpps(1.m) 2^-e exactly, rcpps(1.m) a function of the
// top mantissa bits only -- both probed on the host when the mode is switched on, together with the special cases: zero and
// denormal input give infinity, a result below the normal range is flushed to zero, infinity gives zero, NaN stays NaN (quiet).
__device__ __forceinline__ float rcp_host_table(float z, const RcpTable &rcp) {
  const unsigned u = f2u(z), au = u & 0x7fffffffu, e = au >> 23, m = au & 0x7fffffu;
  const unsigned t = ((const __attribute__((address_space(1))) unsigned *)rcp.table)[m >> rcp.shift];
  const int re = (int)(t >> 23) - ((int)e - 127);  // exponent field of the result
  unsigned r = re >= 1 ? (((unsigned)re << 23) | (t & 0x7fffffu)) : 0u;
  r = e == 0u ? 0x7f800000u : r;
  r = e == 255u ? (m ? (au | 0x00400000u) : 0u) : r;
  return u2f(r | (u & 0x80000000u));
}

// The nibble form (RcpTable::nibbles, round 5): no global-memory gather.  rcpps(1.m) is rebuilt from the device's own reciprocal of
// the midpoint of m's cell -- its top bits, a pure function of the cell index -- plus a signed 4-bit correction from a table
// in LDS (lds_nib: eight cells to a word); exponent and special cases as above.  Bit-identical to rcp_host_table by construction:
// the corrections are (table entry - that very expression) evaluated on this device when the mode is switched on, and the
// switch refuses the form if the expression differs between the two rounding modes the kernel uses it in.
__device__ __forceinline__ unsigned rcp_midpoint_bits(unsigned cell, int shift) {
  return f2u(__builtin_amdgcn_rcpf(u2f(0x3f800000u | (cell << shift) | (1u << (shift - 1)))));
}
// NAN_ANY: a NaN input may give ANY result (the residual pass: a NaN depth makes sx, sy NaN as well, so u, v are NaN and the pixel
// invalid whatever 1 / z is; most wave steps hold such lanes -- unselected pixels -- and must not send the wave down the rare path).
template <bool NAN_ANY>
__device__ __forceinline__ float rcp_host_nibbles(float z, const unsigned *lds_nib, int shift, int unit) {
  const unsigned u = f2u(z), au = u & 0x7fffffffu, e = au >> 23, m = au & 0x7fffffu;
  const unsigned cell = m >> shift;
  const unsigned word = lds_nib[cell >> 3];
  const int corr = (int)(((word >> ((cell & 7u) * 4u)) & 15u) ^ 8u) - 8;  // signed nibble
  const unsigned t = (rcp_midpoint_bits(cell, shift) & ~((1u << unit) - 1u)) + (unsigned)(corr << unit);
  // Common case, branch free: t's exponent field is 126 or 127, so for 1 <= e <= 252 the result's exponent stays a normal one and
  // scaling by 2^-(e - 127) is an integer subtraction on the bit pattern.  Zero / denormal inputs, results that would leave the
  // normal range and infinities / NaNs (e = 0 or e >= 253) take the full rule; the wave branches only if one of its lanes has one.
  unsigned r = t - ((e - 127u) << 23);
  if (__builtin_expect(__builtin_amdgcn_ballot_w64(e - 1u >= 252u && !(NAN_ANY && au > 0x7f800000u)) != 0ull, 0)) {
    const int re = (int)(t >> 23) - ((int)e - 127);
    r = re >= 1 ? (((unsigned)re << 23) | (t & 0x7fffffu)) : 0u;
    r = e == 0u ? 0x7f800000u : r;
    r = e == 255u ? (m ? (au | 0x00400000u) : 0u) : r;
  }
  return u2f(r | (u & 0x80000000u));
}

// Pointers read from a descriptor in memory are generic ("flat") to the compiler; flat loads are slower and cannot be
// counted separately from LDS traffic.  Everything the kernels touch lives in device global memory: say so.
#define DVO_GLOBAL __attribute__((address_space(1)))
typedef float v4f __attribute__((ext_vector_type(4)));               // plain vector types: loadable from any address space
typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f_a8 __attribute__((ext_vector_type(4), aligned(8)));  // 16 bytes that are only 8-byte aligned
typedef const DVO_GLOBAL float *gcf;
// load at (uniform base) + (32-bit unsigned byte offset): selects the scalar-base + 32-bit vector-offset addressing
// mode of global_load, so no 64-bit address arithmetic is spent per access
template <class T, int IMM = 0>
__device__ __forceinline__ T ld_off(const DVO_GLOBAL void *base, unsigned byte_off) {
  return *reinterpret_cast<const DVO_GLOBAL T *>(reinterpret_cast<const DVO_GLOBAL char *>(base) + byte_off + IMM);
}
typedef const DVO_GLOBAL v4f *gcf4;


// what a block needs of the three descriptors, in registers
struct LevelPairDesc {
  const float *r_zsel, *r_i, *r_ix, *r_iy, *tx, *ty;
  const float4 *c_a;
  const float2 *c_b;
  float2 *res[2];
  float *records;
  double *ll_partials;
  float *ll_qmax;
  int *seg_prefix[2];
  int w, h;
  float wc[6], wr[4], ub_x, ub_y;
  RcpTable rcp;  // (only read by the RCP >= 1 kernels)
  const unsigned *rcp_lds;  // (RCP = 2) the block's LDS copy of rcp.nibbles
  float *dbg_w;  // (RCP >= 1 kernels, test instrumentation) SlotDesc::dbg_w
};

// Block-level trace (builds with -DDVO_TRACE_BLOCKS only: scripts/variant.sh trace -DDVO_TRACE_BLOCKS; never in the shipped
// library): every block of k_tick appends {start, after its first step, end} on the 100 MHz constant clock, what it ran and where
// (HW_ID, XCC_ID).  scripts/block_trace.py turns a run's trace into slot occupancy and the phases of a block's life.
#ifdef DVO_TRACE_BLOCKS
struct BlockTrace {
  unsigned long long t0, t_first, t_end;
  unsigned info;   // bits 0..3 steps (log2) | bit 4 likelihood block | bits 8..15 level width / 8 | bits 16..31 blocks of the item
  unsigned hw;     // HW_ID (bits 0..27) | XCC_ID << 28
};
constexpr unsigned kTraceCapacity = 1u << 22;
__device__ BlockTrace g_trace[kTraceCapacity];
__device__ unsigned g_trace_n;
__device__ __forceinline__ unsigned long long trace_clock() { return __builtin_amdgcn_s_memrealtime(); }
__shared__ unsigned long long trace_first;  // set by thread 0 of a residual block after its first step
__shared__ unsigned long long trace_tail;   // -DDVO_TRACE_TAIL: when thread 128 (the ordered combine of the four wave segments) was done
#endif

// ------------------------------------------------------------------------------------------------------------------
// residual pass
// ------------------------------------------------------------------------------------------------------------------

// computeResidualsSse for one reference pixel, dense_tracking_impl.cpp:171-294, split in three so that the 24 gather
// loads of a round (4 pixels x 6) are issued back to back instead of one pixel's loads waiting behind the previous
// pixel's arithmetic.  All three parts run in round-toward-zero.
struct Proj {
  float u, v, sz;
  int base;   // top-left gather index, 0 when the point falls outside
  bool inb;
};
struct Gathered {
  v4f a00, a10, a01, a11;  // {I, Z, Ix, Iy} of the four neighbours
  v4f_a8 b0, b1;           // {Zx, Zy} pairs of the upper and lower row
};

template <int RCP>
__device__ __forceinline__ Proj project_pixel_rtz(const float *kt, const LevelPairDesc &d, float x, float y, float z) {
  // hadd(hadd()) adds lanes (0,1) and (2,3) first (:178-188); the point's w is 1
  const float sx = (kt[0] * x + kt[1] * y) + (kt[2] * z + kt[3]);
  const float sy = (kt[4] * x + kt[5] * y) + (kt[6] * z + kt[7]);
  Proj p;
  p.sz = (kt[8] * x + kt[9] * y) + (kt[10] * z + kt[11]);
  const float rz = RCP == 2   ? rcp_host_nibbles<true>(p.sz, d.rcp_lds, d.rcp.shift, d.rcp.unit)  // :192 (_mm_rcp_ps) ...
                   : RCP == 1 ? rcp_host_table(p.sz, d.rcp)
                              : rcp_toward_zero(p.sz);                                        // ... / the exact quotient
  p.u = sx * rz, p.v = sy * rz;
  // 0 <= u <= w-2 and 0 <= v <= h-2 (:160-161,203); NaN compares false.  (Bitwise and: four compares and three scalar ands;
  // the short-circuit form compiles to an exec-masked region.)
  p.inb = (bool)((int)(p.u >= 0.0f) & (int)(p.u <= d.ub_x) & (int)(p.v >= 0.0f) & (int)(p.v <= d.ub_y));
  const int iu = (int)p.u, iv = (int)p.v;  // truncation == _mm_cvtps_epi32 under RTZ (:195)
  p.base = p.inb ? __mul24(iv, d.w) + iu : 0;  // both factors are below 2^24 for a pixel in bounds: one full-rate v_mad_i32_i24
  return p;
}

__device__ __forceinline__ Gathered gather_pixel(const LevelPairDesc &d, int base) {
  const DVO_GLOBAL void *ca = (const DVO_GLOBAL void *)d.c_a, *cb = (const DVO_GLOBAL void *)d.c_b;
  const unsigned oa0 = (unsigned)base * 16u, oa1 = oa0 + (unsigned)d.w * 16u;  // {I, Z, Ix, Iy}: 16 bytes per pixel
  const unsigned ob0 = (unsigned)base * 8u, ob1 = ob0 + (unsigned)d.w * 8u;    // {Zx, Zy}: 8 bytes per pixel
  Gathered g;
  g.a00 = ld_off<v4f>(ca, oa0), g.a10 = ld_off<v4f, 16>(ca, oa0);
  g.a01 = ld_off<v4f>(ca, oa1), g.a11 = ld_off<v4f, 16>(ca, oa1);
  g.b0 = ld_off<v4f_a8>(cb, ob0);
  g.b1 = ld_off<v4f_a8>(cb, ob1);
  return g;
}

// Cache policy of k_tick's streams, chosen here and nowhere else:
//  - the current pyramid's gather planes (gather_pixel above) and the reference pyramid's compacted arrays (the six prefetched
//    dword loads of a step) are shared by every resident pair of that frame: default policy, they are what should stay cached;
//  - the residual spill, its one re-read by the likelihood pass of a later tick and the per-block records are private to a pair
//    and touched exactly once per direction: non-temporal (the `nt` bit of global_store / global_load), so that a sixth of the
//    tick's traffic does not age the shared lines out of L2 and the Infinity Cache.  An nt store is an ordinary write-back store
//    as far as visibility goes (the consumer is a later launch), an nt load bypasses only L1, where a streamed line has no reuse.
template <class T>
__device__ __forceinline__ void st_once(DVO_GLOBAL T *p, const T v) {
  __builtin_nontemporal_store(v, p);
}
template <class T>
__device__ __forceinline__ T ld_once(const DVO_GLOBAL T *p) {
  return __builtin_nontemporal_load(p);
}

// ZERO_E: also zero the gradient terms of an invalid pixel (the register-accumulator form needs that; the staged forms scale
// them by a zero weight with a multiply whose 0 * anything is 0, so the four selects are saved)
template <bool ZERO_E>
__device__ __forceinline__ void finish_pixel_rtz(const LevelPairDesc &d, const Proj &p, const Gathered &g, float z, float ri,
                                                 float rix, float riy, float &r0, float &r1, float &e2, float &e3, float &e4,
                                                 float &e5, bool &valid) {
  // u - (float)(int)u (:211-216): for a point in bounds (u >= 0) that is u - floor(u), an exact difference: v_fract_f32
  const float w1u = __builtin_amdgcn_fractf(p.u), w1v = __builtin_amdgcn_fractf(p.v);
  const float w0u = 1.0f - w1u, w0v = 1.0f - w1v;
  // bilinear blend, per channel: w0v*(w0u*c00 + w1u*c10) + w1v*(w0u*c01 + w1u*c11)  (:227-258)
#define DVO_BLEND(c00, c10, c01, c11) ((w0v * (w0u * (c00) + w1u * (c10))) + (w1v * (w0u * (c01) + w1u * (c11))))
  const float ci = DVO_BLEND(g.a00.x, g.a10.x, g.a01.x, g.a11.x);
  const float cz = DVO_BLEND(g.a00.y, g.a10.y, g.a01.y, g.a11.y);
  const float cix = DVO_BLEND(g.a00.z, g.a10.z, g.a01.z, g.a11.z);
  const float ciy = DVO_BLEND(g.a00.w, g.a10.w, g.a01.w, g.a11.w);
  const float czx = DVO_BLEND(g.b0.x, g.b0.z, g.b1.x, g.b1.z);
  const float czy = DVO_BLEND(g.b0.y, g.b0.w, g.b1.y, g.b1.w);
#undef DVO_BLEND
  // any NaN among the blended channels rejects the point (:261); channels 6,7 are always 0
  // (one unordered compare tests two channels)
  const bool has_nan = __builtin_isunordered(ci, cz) || __builtin_isunordered(cix, ciy) || __builtin_isunordered(czx, czy);
  // e = wcur * cur + wref * ref', ref' = {I, transformed depth, Ix, Iy} (:269-271)
  const float t0 = d.wc[0] * ci + d.wr[0] * ri;
  const float t1 = d.wc[1] * cz + d.wr[1] * p.sz;
  // occlusion test (:275) with depthStdDevZ (:122-128) of the reference depth
  float s = z - 0.4f;
  s = 0.0012f + (0.0019f * s) * s;
  valid = p.inb && !has_nan && (t1 > -20.0f * s);
  r0 = valid ? t0 : 0.0f;
  r1 = valid ? t1 : 0.0f;
  e2 = d.wc[2] * cix + d.wr[2] * rix;
  e3 = d.wc[3] * ciy + d.wr[3] * riy;
  e4 = d.wc[4] * czx;  // wref is 0 for the depth derivatives (dense_tracking.cpp:217-220)
  e5 = d.wc[5] * czy;
  if (ZERO_E) e2 = valid ? e2 : 0.0f, e3 = valid ? e3 : 0.0f, e4 = valid ? e4 : 0.0f, e5 = valid ? e5 : 0.0f;
}

typedef float v4acc __attribute__((ext_vector_type(4)));
// The Gram matrix of the staged 16-vector v = sqrt(w) (Ja[0..5], Jb[0..5], r0, r1, 0, 0), as 4 x 4 tiles of 4-component chunks:
// of the 16 chunk pairs only the 9 with ci <= cj < 4, ci < 3 hold moments (the tile is symmetric, r r^T is not needed).
// v_mfma_f32_4x4x1_16b_f32 forms sixteen independent 4 x 4 outer products per instruction in 8 issue cycles (measured 8.9;
// the 16x16x4 form: 33 for 4 points x 256 products, and matrix and vector instructions of a SIMD do NOT overlap on gfx950 --
// scripts/probes/mfma_valu_coexec.hip, mfma_4x4_blocks.hip): block b of an instruction is point 16 g + b of the step, so 4 x 9 = 36
// instructions (320 cycles) do the work of sixteen 16x16x4 ones (530).  DVO_GRAM_BLOCKS=0 builds the 16x16x4 form.
#ifndef DVO_GRAM_BLOCKS
#define DVO_GRAM_BLOCKS 1
#endif
constexpr int kGramPairs = 9;
// tile index of the chunk pair (ci <= cj): (0,0) (0,1) (0,2) (0,3) (1,1) (1,2) (1,3) (2,2) (2,3)
__host__ __device__ constexpr int gram_pair(int ci, int cj) { return ci == 0 ? cj : ci == 1 ? 3 + cj : 5 + cj; }

// wave-local LDS hand-off: the LDS queue of a wave is in order, the fences only pin the compiler
#define DVO_WAVE_LDS_SYNC()                                 \
  do {                                                      \
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  \
    __builtin_amdgcn_wave_barrier();                        \
  } while (0)

// Timing-only ablation builds (scripts/ablate.sh: -DDVO_ABLATE=<mask>); never defined in the shipped library.
// 1: no LDS staging / MFMA   2: no gather loads   4: no rank / pair-sum logic   8: no residual spill store
// 16: no pixel steps at all (prologue + epilogue only)   32: no epilogue (reductions, block record)
// 64: epilogue without the seven wave reductions   128: without the moment sums of the four waves   256: without the ordered
// combine of the four wave segments
#ifndef DVO_ABLATE
#define DVO_ABLATE 0
#endif
#define DVO_KEEP(x) asm volatile("" ::"v"(x))

// The fused residual pass.  It walks the SELECTED pixels of the reference level in scan order -- the compacted arrays k_compact
// builds, as the reference walks PointSelection's dense array (dense_tracking_impl.cpp:169-171) -- so its cost follows the
// selection, not the image (round 5, end; until then every pixel of the level took a lane and unselected ones carried a NaN depth).
// A wave walks its segment in steps of 64 consecutive points, one point per lane: neighbouring selected pixels, so that every
// gather instruction of a step touches ~64 neighbouring pixels of the current image (whole cache lines, reused by the
// other three neighbour loads of the same step while they are still in L1).
//
// ACC 0: the 87 moments live in 87 fp32 registers per lane (fma), reduced across the wave with DPP at the end.
// ACC 1: the moments are the Gram matrix G = sum_p w_p v_p v_p^T of v = [Ja(6), Jb(6), r0, r1, 0, 0]; sqrt(w) v is staged
//        through LDS (lane-per-point -> lane-per-component) and accumulated by v_mfma_f32_16x16x4_f32 into 2 x 4
//        registers.  The MFMA sums over the points itself, so no 87-value wave reduction is needed and the kernel fits
//        4 waves per SIMD (the 87-register form is capped at 2).
//        (round 4: as nine 4 x 4 tiles on v_mfma_f32_4x4x1_16b_f32 into 9 x 4 registers, DVO_GRAM_BLOCKS above -- the default;
//        round 2's first 4x4 build had spills at four waves per SIMD and was dropped then.)
// (Measured and removed in round 3, DESIGN.md section 10: a five-waves-per-SIMD build, physical blocks walking several logical
// ones, item tables in device memory.)
// RCP 0 (default): 1 / z of the projection is the exactly truncated quotient, the t-distribution weight 7 v_rcp_f32(5 + d).
// RCP 1 (dvo_amd_set_reciprocal_mode): both reciprocals are the host's _mm_rcp_ps, bit for bit (dense_tracking_impl.cpp:192,700),
//       from a table in global memory; RCP 2: the same function from a 2 KiB correction table in LDS (rcp_host_nibbles).
template <int ACC, int RCP>
__device__ void residual_pass(const TickItem &it, const LevelPairDesc &d_in, const int lb) {
  LevelPairDesc d = d_in;
  __shared__ unsigned rcp_lds[RCP == 2 ? kRcpNibbleWordsMax : 1];
  if (RCP == 2) {
    // every block copies the corrections (L2-resident, 2 KiB) next to its staging area; the first projection waits for them
    const int words = (1 << (23 - d.rcp.shift)) >> 3;
    for (int i = threadIdx.x; i < words; i += kBlockThreads) rcp_lds[i] = ((const DVO_GLOBAL unsigned *)d.rcp.nibbles)[i];
    __syncthreads();
    d.rcp_lds = rcp_lds;
  }
  constexpr int kBufs = 2;
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  // the wave's number as a scalar, for the staging addresses formed inside the steps and after them: as a vector value the
  // wave's staging offset is one more register that lives through the whole pass
  const int wave_s = __builtin_amdgcn_readfirstlane(wave);
  const int seg = lb * kWavesPerBlock + wave;
  const int steps = item_res_steps(it);  // a segment is steps * 64 points
  unsigned idx = (unsigned)(seg * (kStepPx * steps) + lane);  // a POINT of the compacted selection (k_compact), not a pixel

  float acc[ACC == 0 ? kNumAcc : 1];
#pragma unroll
  for (int i = 0; i < (ACC == 0 ? kNumAcc : 1); ++i) acc[i] = 0.0f;
  v4acc gram_a = {0.0f, 0.0f, 0.0f, 0.0f}, gram_b = {0.0f, 0.0f, 0.0f, 0.0f};
  v4acc gram_p[kGramPairs];  // (DVO_GRAM_BLOCKS) one 4 x 4 tile per needed pair of 4-component chunks, 16 point classes each
#pragma unroll
  for (int k = 0; k < kGramPairs; ++k) gram_p[k] = v4acc{0.0f, 0.0f, 0.0f, 0.0f};
  // staging for the MFMA operands: [wave][point = lane][16 components], 16-byte chunks XOR-swizzled by point
  __shared__ __attribute__((aligned(16))) float stage[ACC >= 1 ? kWavesPerBlock * kBufs * kWave * 16 : 4];
  float S0[3] = {0.0f, 0.0f, 0.0f}, S1[3] = {0.0f, 0.0f, 0.0f};
  float first_w = 0.0f;
  int run_count = 0;                        // wave uniform
  // The pair quirk needs, for every valid pixel, the residual of the valid pixel before it in scan order.  Each wave keeps
  // the valid residuals of the current step compacted in LDS: slot 0 = the last valid pixel of earlier steps (zeros at
  // the start of a segment), slot 1 + k = the k-th valid pixel of this step; a pixel with k valid pixels below it in the
  // wave finds its predecessor in slot k.  (Ballot / mbcnt give k; no cross-lane shuffles, no carry registers.)
  __shared__ __attribute__((aligned(8))) v2f pair_slots[kWavesPerBlock][kWave + 2];
  v2f *const slots = pair_slots[wave];
  if (lane == 0) slots[0] = v2f{0.0f, 0.0f};

  // K*T lives in vector registers: as scalars the 12 values do not fit next to the descriptors, and the compiler re-reads
  // them from the kernel arguments inside every step, with a full scalar-memory wait in front of the projection
  float kt[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    kt[i] = it.kt[i];
    if (DVO_KT_SGPR)
      asm volatile("" : "+s"(kt[i]));
    else
      DVO_OPAQUE(kt[i]);
  }
  const bool unit_w = (it.flags & kItemUnitWeights) != 0;
  const float P0 = it.P[0], P1 = it.P[1], P2 = it.P[2], P3 = it.P[3];
  const DVO_GLOBAL void *const p_z = (const DVO_GLOBAL void *)d.r_zsel, *const p_i = (const DVO_GLOBAL void *)d.r_i,
                         *const p_ix = (const DVO_GLOBAL void *)d.r_ix, *const p_iy = (const DVO_GLOBAL void *)d.r_iy,
                         *const p_tx = (const DVO_GLOBAL void *)d.tx, *const p_ty = (const DVO_GLOBAL void *)d.ty;
  DVO_GLOBAL char *const p_res = (DVO_GLOBAL char *)((it.flags & kItemResBuf) ? d.res[1] : d.res[0]);  // no dynamic index: keeps d in registers

  // the points of the step about to be processed (depth, intensity, derivatives, ray: six coalesced dword loads, issued behind
  // the Gram stage of the step before -- about two thirds of a step ahead of their first use); all accesses are uniform base +
  // 32-bit offset
  // (a two-step lead with two alternating register sets was measured: +10 VGPRs, +9 VALU per step, no gain in or out of cache)
  // (the first step's loads stand in each arm of the step-count branch below -- load_first: issued once in front of the branch,
  //  the six values are live across the code of the arm not taken, and at 128 VGPRs the register allocator spills them)
  float n_z, n_i, n_ix, n_iy, n_tx, n_ty;  // (n_tx, n_ty: the point's ray; padding: zeros under a NaN depth)
  auto load_first = [&](const bool opaque) __attribute__((always_inline)) {
    unsigned at = idx;
    if (opaque) DVO_OPAQUE(at);  // keeps the two arms' loads apart
    n_z = ld_off<float>(p_z, 4u * at), n_i = ld_off<float>(p_i, 4u * at), n_ix = ld_off<float>(p_ix, 4u * at),
    n_iy = ld_off<float>(p_iy, 4u * at);
    n_tx = ld_off<float>(p_tx, 4u * at), n_ty = ld_off<float>(p_ty, 4u * at);
  };

  // Operand fetch of the Gram-matrix accumulation: lane l supplies component l & 15 of points 4 m + (l >> 4), m = 0..15, of
  // the 64 points a step staged.  With the write swizzle below, chunk (comp >> 2) of point p sits at chunk position
  // (comp >> 2) ^ ((p >> 1) & 3) = cb for even m and cb ^ 2 for odd m (cb = (comp >> 2) ^ (l >> 5)): two lane-constant
  // offsets plus compile-time immediates, no per-step address arithmetic.
  const int g_comp = lane & 15, g_sub = lane >> 4, g_cb = (g_comp >> 2) ^ (g_sub >> 1);
  const float *const g_even = stage + (wave * kBufs * kWave + g_sub) * 16 + ((g_cb << 2) | (g_comp & 3));
  const float *const g_odd = stage + (wave * kBufs * kWave + g_sub) * 16 + (((g_cb ^ 2) << 2) | (g_comp & 3));
  // The 4 x 4 form: lane l supplies component l & 3 of chunk c of point 16 g + (l >> 2) as the A (row) and B (column) operand of
  // the tiles chunk c takes part in.  The point's swizzle ((p >> 1) & 3 = (l >> 3) & 3, the same for every g) makes the four
  // chunk positions lane constants; g and the buffer are immediates.  Eight consecutive points x one chunk = 32 distinct banks.
  const int b_swz = (lane >> 3) & 3;
  const float *const b_base = stage + (wave * kBufs * kWave + (lane >> 2)) * 16 + (lane & 3);
  const float *const b_c0 = b_base + 4 * (0 ^ b_swz), *const b_c1 = b_base + 4 * (1 ^ b_swz), *const b_c2 = b_base + 4 * (2 ^ b_swz),
                     *const b_c3 = b_base + 4 * (3 ^ b_swz);
  auto gram_from_stage = [&](const int q) __attribute__((always_inline)) {
    if (DVO_GRAM_BLOCKS) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int off = (q & (kBufs - 1)) * kWave * 16 + g * 16 * 16;
        const float x0 = b_c0[off], x1 = b_c1[off], x2 = b_c2[off], x3 = b_c3[off];
        gram_p[0] = __builtin_amdgcn_mfma_f32_4x4x1f32(x0, x0, gram_p[0], 0, 0, 0);
        gram_p[1] = __builtin_amdgcn_mfma_f32_4x4x1f32(x0, x1, gram_p[1], 0, 0, 0);
        gram_p[2] = __builtin_amdgcn_mfma_f32_4x4x1f32(x0, x2, gram_p[2], 0, 0, 0);
        gram_p[3] = __builtin_amdgcn_mfma_f32_4x4x1f32(x0, x3, gram_p[3], 0, 0, 0);
        gram_p[4] = __builtin_amdgcn_mfma_f32_4x4x1f32(x1, x1, gram_p[4], 0, 0, 0);
        gram_p[5] = __builtin_amdgcn_mfma_f32_4x4x1f32(x1, x2, gram_p[5], 0, 0, 0);
        gram_p[6] = __builtin_amdgcn_mfma_f32_4x4x1f32(x1, x3, gram_p[6], 0, 0, 0);
        gram_p[7] = __builtin_amdgcn_mfma_f32_4x4x1f32(x2, x2, gram_p[7], 0, 0, 0);
        gram_p[8] = __builtin_amdgcn_mfma_f32_4x4x1f32(x2, x3, gram_p[8], 0, 0, 0);
      }
      return;
    }
#pragma unroll
    for (int m = 0; m < 16; m += 2) {
      const float va = g_even[(q & (kBufs - 1)) * kWave * 16 + 64 * m];
      const float vb = g_odd[(q & (kBufs - 1)) * kWave * 16 + 64 * (m + 1)];
      gram_a = __builtin_amdgcn_mfma_f32_16x16x4f32(va, va, gram_a, 0, 0, 0);
      gram_b = __builtin_amdgcn_mfma_f32_16x16x4f32(vb, vb, gram_b, 0, 0, 0);
    }
  };

  // One step = 64 consecutive points of the compacted selection, one per lane.  The loop is unrolled by two (a segment always has a multiple of four
  // steps) so that the staging-buffer parity q is a compile-time constant and the one-step-ahead prefetch registers need
  // no rotation moves.
  auto do_step = [&](const int step, const int q, const bool prefetch) __attribute__((always_inline)) {
    const unsigned cur_idx = idx;
    // ---- round-to-nearest: reference point = pixel ray * depth (RgbdCamera::buildPointCloud, rgbd_image.cpp:245-262)
    float z = n_z, ri = n_i, rix = n_ix, riy = n_iy;
    float x = n_tx * z, y = n_ty * z;
    // the next step's reference scalars are prefetched behind the Gram stage below (prefetch_next) and consumed in the next step
    idx += kWave;
    auto prefetch_next = [&]() __attribute__((always_inline)) {
      n_z = ld_off<float>(p_z, 4u * idx), n_i = ld_off<float>(p_i, 4u * idx), n_ix = ld_off<float>(p_ix, 4u * idx),
      n_iy = ld_off<float>(p_iy, 4u * idx);
      n_tx = ld_off<float>(p_tx, 4u * idx), n_ty = ld_off<float>(p_ty, 4u * idx);
    };

    // ---- switch to round-toward-zero: every float that crosses is made opaque on both sides of the s_setreg
    DVO_OPAQUE(x); DVO_OPAQUE(y); DVO_OPAQUE(z); DVO_OPAQUE(ri); DVO_OPAQUE(rix); DVO_OPAQUE(riy);
    round_toward_zero();
    DVO_OPAQUE(x); DVO_OPAQUE(y); DVO_OPAQUE(z); DVO_OPAQUE(ri); DVO_OPAQUE(rix); DVO_OPAQUE(riy);
    float r0, r1, e2, e3, e4, e5;
    bool ok;
    {
      const Proj p = project_pixel_rtz<RCP>(kt, d, x, y, z);
      Gathered g;
      if (DVO_ABLATE & 2) {
        const v4f c = {p.u, 1.5f, p.v, 0.25f};
        g.a00 = c, g.a10 = c, g.a01 = c, g.a11 = c, g.b0 = c, g.b1 = c;
        DVO_KEEP(p.base);
      } else {
        g = gather_pixel(d, p.base);
        // Pin the six gather loads in front of the Gram stage: left to itself the scheduler sinks them, with their offset
        // arithmetic, behind 28 to 31 of the 36 v_mfma, and the gather latency then starts where the matrix work ends.
        if (ACC >= 1 && !(DVO_ABLATE & 1) && step > 0) __builtin_amdgcn_sched_barrier(0);
      }

      // The gathers are in flight (the barrier above): feed the matrix pipe with the vectors the PREVIOUS step staged
      // (v_mfma_f32 ignores MODE.FP_ROUND -- probed on gfx950, scripts/probes/mfma_round.hip -- so it may sit in
      // the toward-zero window).  The 36 instructions -- 36 x 8 = 288 issue cycles by the cycle model of DESIGN.md section 4.1,
      // a model figure, not a measurement -- now run under the gather latency instead of in front of it; the first use of the
      // gathered data (v_fract, the blend) follows the last v_mfma.
      if (ACC >= 1 && !(DVO_ABLATE & 1) && step > 0) {
        gram_from_stage(q ^ 1);
        __builtin_amdgcn_sched_barrier(0);
      }
      // The next step's reference scalars go out here, not at the top of the step: across the Gram stage the 24 gathered
      // registers and the 36 accumulators are live together, and six prefetch targets on top of them cost scratch at 128
      // VGPRs.  They still lead their first use by the blend, the weights, the Jacobian and the staging: ~2/3 of a step.
      if (prefetch) prefetch_next();
      finish_pixel_rtz<ACC == 0>(d, p, g, z, ri, rix, riy, r0, r1, e2, e3, e4, e5, ok);
    }
    // ---- back to round-to-nearest
    DVO_OPAQUE(r0); DVO_OPAQUE(r1); DVO_OPAQUE(e2); DVO_OPAQUE(e3); DVO_OPAQUE(e4); DVO_OPAQUE(e5);
    DVO_OPAQUE(x); DVO_OPAQUE(y); DVO_OPAQUE(z);
    round_to_nearest();
    DVO_OPAQUE(r0); DVO_OPAQUE(r1); DVO_OPAQUE(e2); DVO_OPAQUE(e3); DVO_OPAQUE(e4); DVO_OPAQUE(e5);
    DVO_OPAQUE(x); DVO_OPAQUE(y); DVO_OPAQUE(z);

    // spill the residual of this iteration for the log-likelihood pass (NaN marks an invalid pixel)
    {
      const float qnan = u2f(0x7fc00000u);
      v2f sv;
      sv.x = ok ? r0 : qnan, sv.y = ok ? r1 : qnan;
      if (DVO_ABLATE & 8) {
        DVO_KEEP(sv.x);
        DVO_KEEP(sv.y);
      } else {
        st_once(reinterpret_cast<DVO_GLOBAL v2f *>(p_res + 8u * cur_idx), sv);
      }
    }

    // Branch free from here: an invalid pixel carries weight 0, zero residuals and a harmless point (exact zeros).
    // computeWeightsSse / computeWeight: w = (2+5)/(5 + r^T P r), mean 0 (dense_tracking_impl.cpp:640-707)
    float wgt = 1.0f;
    if (!unit_w) {
      // (round-to-nearest section: in the default mode fused multiply-adds are fine here, only the toward-zero stage is
      //  bit-matched; the host-rcpps kernels form the distance as computeWeightsSse does, product by product (:669-697), so that
      //  every weight is the reference's bit for bit)
      const float t0 = RCP ? r0 * P0 + r1 * P1 : __builtin_fmaf(r0, P0, r1 * P1);
      const float t1 = RCP ? r0 * P2 + r1 * P3 : __builtin_fmaf(r0, P2, r1 * P3);
      const float dd = RCP ? t0 * r0 + t1 * r1 : __builtin_fmaf(t0, r0, t1 * r1);
      wgt = 7.0f * (RCP == 2   ? rcp_host_nibbles<true>(5.0f + dd, d.rcp_lds, d.rcp.shift, d.rcp.unit)
                    : RCP == 1 ? rcp_host_table(5.0f + dd, d.rcp)
                               : __builtin_amdgcn_rcpf(5.0f + dd));
    }
    wgt = ok ? wgt : 0.0f;
    if (RCP && d.dbg_w) ((DVO_GLOBAL float *)d.dbg_w)[cur_idx] = ok ? wgt : u2f(0x7fc00000u);  // (dvo_amd_debug_weights only)

    // Jacobians at the untransformed reference point (dense_tracking.cpp:333-339,448-476)
    // (Formed from the pixel's ray instead -- x / z is tx, y / z is ty: five instructions fewer, same Jacobian to an ulp -- the
    //  batch ran at the same 47.0 k pairs/s, three interleaved runs, gpurun_out/r4f: not kept, the arithmetic stays as it was.)
    x = ok ? x : 0.0f, y = ok ? y : 0.0f, z = ok ? z : 1.0f;
    const float iz = __builtin_amdgcn_rcpf(z);
    const float iz2 = iz * iz;
    const float j02 = -x * iz2, j12 = -y * iz2;
    const float j03 = j02 * y, j13 = __builtin_fmaf(j12, y, -1.0f);
    const float j04 = __builtin_fmaf(-j02, x, 1.0f), j14 = -j03;
    const float j05 = -y * iz, j15 = x * iz;
    // The staged forms accumulate sqrt(w) v: the factor goes onto the four gradient terms and the three constants of Jz
    // before the 2 x 6 rows are formed (8 multiplies instead of 14 on the finished rows).  v_mul_legacy_f32: 0 * x = 0 for
    // every x, so the zero weight of an invalid pixel also wipes whatever its gradient terms hold (NaN included).
    const float sw = ACC == 0 ? 1.0f : __builtin_amdgcn_sqrtf(wgt);
    const float g2 = ACC == 0 ? e2 : mul_legacy(sw, e2), g3 = ACC == 0 ? e3 : mul_legacy(sw, e3);
    const float g4 = ACC == 0 ? e4 : mul_legacy(sw, e4), g5 = ACC == 0 ? e5 : mul_legacy(sw, e5);
    const float swx = sw * x, swy = sw * y;
    float Ja[6], Jb[6];
    Ja[0] = g2 * iz;
    Ja[1] = g3 * iz;
    Ja[2] = __builtin_fmaf(g2, j02, g3 * j12);
    Ja[3] = __builtin_fmaf(g2, j03, g3 * j13);
    Ja[4] = __builtin_fmaf(g2, j04, g3 * j14);
    Ja[5] = __builtin_fmaf(g2, j05, g3 * j15);
    Jb[0] = g4 * iz;
    Jb[1] = g5 * iz;
    Jb[2] = __builtin_fmaf(g4, j02, __builtin_fmaf(g5, j12, -sw));
    Jb[3] = __builtin_fmaf(g4, j03, __builtin_fmaf(g5, j13, -swy));
    Jb[4] = __builtin_fmaf(g4, j04, __builtin_fmaf(g5, j14, swx));
    Jb[5] = __builtin_fmaf(g4, j05, g5 * j15);
    // A += J^T (w P) J and b -= J^T (w P) r are linear in P: accumulate the P-free moments (87 sums)
    if (ACC == 0) {
      float wa[6], wb[6];
#pragma unroll
      for (int i = 0; i < 6; ++i) wa[i] = wgt * Ja[i], wb[i] = wgt * Jb[i];
      int t = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j, ++t) {
          acc[kAccAA + t] = __builtin_fmaf(wa[i], Ja[j], acc[kAccAA + t]);
          acc[kAccAB + t] = __builtin_fmaf(wa[i], Jb[j], __builtin_fmaf(wb[i], Ja[j], acc[kAccAB + t]));
          acc[kAccBB + t] = __builtin_fmaf(wb[i], Jb[j], acc[kAccBB + t]);
        }
        acc[kAccAR0 + i] = __builtin_fmaf(wa[i], r0, acc[kAccAR0 + i]);
        acc[kAccAR1 + i] = __builtin_fmaf(wa[i], r1, acc[kAccAR1 + i]);
        acc[kAccBR0 + i] = __builtin_fmaf(wb[i], r0, acc[kAccBR0 + i]);
        acc[kAccBR1 + i] = __builtin_fmaf(wb[i], r1, acc[kAccBR1 + i]);
      }
    } else if (DVO_ABLATE & 1) {
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        DVO_KEEP(Ja[i]);
        DVO_KEEP(Jb[i]);
      }
      DVO_KEEP(wgt);
    } else {
      // stage sqrt(w) * v for this lane's pixel; chunk c of point p sits at chunk position c ^ ((p >> 1) & 3).
      // Two buffers alternate: the matrix pipe consumes this one during the NEXT step (see above).
      float *buf = stage + ((wave_s * kBufs + (q & (kBufs - 1))) * kWave) * 16;
      v4f *row = reinterpret_cast<v4f *>(buf + lane * 16);
      const int swz = (lane >> 1) & 3;
      v4f c0 = {Ja[0], Ja[1], Ja[2], Ja[3]};  // the rows carry sqrt(w) already
      v4f c1 = {Ja[4], Ja[5], Jb[0], Jb[1]};
      v4f c2 = {Jb[2], Jb[3], Jb[4], Jb[5]};
      v4f c3 = {sw * r0, sw * r1, 0.0f, 0.0f};
      // the LDS queue of a wave is in order: these writes land after the reads of two steps ago and before the reads of
      // the next step; the fences only stop the compiler from reordering across them
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
      row[0 ^ swz] = c0;
      row[1 ^ swz] = c1;
      row[2 ^ swz] = c2;
      row[3 ^ swz] = c3;
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }

    if (DVO_ABLATE & 4) {
      S0[0] += wgt * r0;
      run_count += __popcll(__ballot(ok));
      return;
    }
    // ---- rank of every valid pixel in scan order within this wave's segment (needed by the pair quirk Q5)
    const unsigned long long bk = __builtin_amdgcn_ballot_w64(ok);  // (__ballot() takes the flag through a vector register and back)
    const int pos = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(bk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bk, 0u));
    const int rank = run_count + pos;
    const int n_here = __popcll(bk);
    DVO_WAVE_LDS_SYNC();
    if (ok) slots[pos + 1] = v2f{r0, r1};
    DVO_WAVE_LDS_SYNC();
    const v2f prev = slots[pos];  // the valid pixel before this one (invalid lanes read a valid slot too: weight 0)
    DVO_WAVE_LDS_SYNC();
    if (n_here) slots[0] = slots[n_here];  // every lane moves the same value: the carry for the next step
    {
      // computeScaleSse with Q5: a pair (2j, 2j+1) contributes (w_2j + w_2j+1) r_2j r_2j^T (:603-621).
      // S0 assumes this segment starts on an even global rank, S1 on an odd one.  Invalid pixels have weight 0.
      // the segment's first valid pixel reads the zeros slot 0 starts with, so its "predecessor" products vanish.
      // (the residual is picked before it is squared: four selects instead of six)
      const bool odd = (rank & 1) != 0;
      const float a0 = odd ? prev.x : r0, a1 = odd ? prev.y : r1;  // what the even-start hypothesis weights at this pixel
      const float b0 = odd ? r0 : prev.x, b1 = odd ? r1 : prev.y;  // ... the odd-start hypothesis
      S0[0] = __builtin_fmaf(wgt, a0 * a0, S0[0]);
      S0[1] = __builtin_fmaf(wgt, a0 * a1, S0[1]);
      S0[2] = __builtin_fmaf(wgt, a1 * a1, S0[2]);
      S1[0] = __builtin_fmaf(wgt, b0 * b0, S1[0]);
      S1[1] = __builtin_fmaf(wgt, b0 * b1, S1[1]);
      S1[2] = __builtin_fmaf(wgt, b1 * b1, S1[2]);
      // first valid pixel of the segment: its partner (if any) lives in an earlier segment
      first_w = (ok && rank == 0) ? wgt : first_w;
    }
    run_count += n_here;
  };
  // the last pair of steps is peeled so that "is there a next step to prefetch" is a compile-time fact in every copy
  if (!(DVO_ABLATE & 16)) {  // (ablation 16: prologue + epilogue only)
    if (steps == 1) {
      load_first(true);
      do_step(0, 1, false);  // a one-step segment stages into buffer 1, which the epilogue consumes
#if defined(DVO_TRACE_BLOCKS) && !defined(DVO_TRACE_DESC)
      if (threadIdx.x == 0) trace_first = trace_clock();
#endif
    } else {
#ifdef DVO_TRACE_BLOCKS
      bool marked = false;
#endif
      load_first(false);
      for (int step = 0; step + 2 < steps; step += 2) {
        do_step(step, 0, true);
#if defined(DVO_TRACE_BLOCKS) && !defined(DVO_TRACE_DESC)
        if (!marked && threadIdx.x == 0) trace_first = trace_clock();
        marked = true;
#endif
        do_step(step + 1, 1, true);
      }
      do_step(steps - 2, 0, true);
#if defined(DVO_TRACE_BLOCKS) && !defined(DVO_TRACE_DESC)
      if (!marked && threadIdx.x == 0) trace_first = trace_clock();
#endif
      do_step(steps - 1, 1, false);
    }
  }

  if (DVO_ABLATE & 32) {  // (ablation 32: no epilogue -- keep the accumulators alive, write nothing)
    float keep = S0[0] + S1[0] + first_w + gram_a[0] + gram_b[0] + (float)run_count;
    for (int k = 0; k < kGramPairs; ++k) keep += gram_p[k][0];
    DVO_KEEP(keep);
    return;
  }
  if (ACC >= 1 && !(DVO_ABLATE & 1) && steps > 0) gram_from_stage(1);  // the last step (odd index) staged into buffer 1

  // ---- wave reduction, then the four waves of the block through LDS
  __shared__ float sm[kWavesPerBlock][kRecStride];
  if (ACC == 0) {
#pragma unroll
    for (int i = 0; i < kNumAcc; ++i) {
      const float s = wave_sum_to_lane63(acc[i]);
      if (lane == 63) sm[wave][kRecAcc + i] = s;
    }
  } else {
    // C/D layout of the 16x16 MFMA: register r of lane l is G[row = (l>>4)*4 + r][col = l&15]
    // into the start of the wave's own staging area (its reads of it are behind it in the in-order LDS queue)
    float *gsm = stage + wave_s * kBufs * kWave * 16;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (DVO_GRAM_BLOCKS) {
      // D layout of the 4 x 4 form: register r of lane l = tile[block l >> 2][row r][column l & 3].  The four blocks of a
      // 16-lane row are added in registers, (b0 + b1) + (b2 + b3); the four rows and the four waves by the threads that
      // gather the moments below: gsm[tile][row of lanes][column][row] (one 16-byte store per tile)
#pragma unroll
      for (int k = 0; k < kGramPairs; ++k) {
        v4acc t = gram_p[k];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = t[r];
          v += dpp_read<0x124, 0xF>(v);  // row_ror:4
          v += dpp_read<0x128, 0xF>(v);  // row_ror:8
          t[r] = v;
        }
        if ((lane & 12) == 0) *reinterpret_cast<v4f *>(gsm + ((k * 4 + (lane >> 4)) * 4 + (lane & 3)) * 4) = v4f{t[0], t[1], t[2], t[3]};
      }
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) gsm[((lane >> 4) * 4 + r) * 16 + (lane & 15)] = gram_a[r] + gram_b[r];
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const float s0 = (DVO_ABLATE & 64) ? S0[i] : wave_sum_to_lane63(S0[i]);
    const float s1 = (DVO_ABLATE & 64) ? S1[i] : wave_sum_to_lane63(S1[i]);
    if (lane == 63) sm[wave][kRecS0 + i] = s0, sm[wave][kRecS1 + i] = s1;
  }
  {
    const float fw = (DVO_ABLATE & 64) ? first_w : wave_sum_to_lane63(first_w);
    if (lane == 63) {
      const v2f last = slots[0];  // the last valid residual of the segment (zeros if there is none)
      sm[wave][kRecFirstW] = fw;
      sm[wave][kRecCount] = u2f((unsigned)run_count);
      sm[wave][kRecLastR] = last.x;
      sm[wave][kRecLastR + 1] = last.y;
    }
  }
  // which Gram-matrix entries make up moment `tid` (rows/cols 0-5 = Ja, 6-11 = Jb, 12 = r0, 13 = r1): worked out while the
  // other waves are still on their way to the barrier
  const int tid = threadIdx.x;
  int e0 = 0, e1 = -1;
  if (ACC >= 1 && tid < kNumAcc) {
    if (tid < kAccAR0) {
      const int kind = tid / 21;
      int t = tid - kind * 21, i = 0;
      while (t >= 6 - i) t -= 6 - i, ++i;
      const int j = i + t;
      if (kind == 0) {
        e0 = i * 16 + j;
      } else if (kind == 1) {
        e0 = i * 16 + 6 + j, e1 = j * 16 + 6 + i;
      } else {
        e0 = (6 + i) * 16 + 6 + j;
      }
    } else {
      const int q = tid - kAccAR0, grp = q / 6, i = q - grp * 6;  // AR0, AR1, BR0, BR1
      e0 = ((grp >> 1) * 6 + i) * 16 + 12 + (grp & 1);
    }
    if (DVO_GRAM_BLOCKS) {  // entry (row, column), row <= column chunk-wise -> offset of gsm[tile][0][column & 3][row & 3]
      auto at = [](const int e) { return ((gram_pair((e >> 4) >> 2, (e & 15) >> 2) * 4) * 4 + (e & 3)) * 4 + ((e >> 4) & 3); };
      e0 = at(e0);
      if (e1 >= 0) e1 = at(e1);
    }
  }
  __syncthreads();

  DVO_GLOBAL float *rec = (DVO_GLOBAL float *)d.records + (size_t)lb * kRecStride;
  if ((DVO_ABLATE & 128) && tid < kNumAcc) {
    st_once(rec + kRecAcc + tid, stage[tid]);
  } else if ((DVO_ABLATE & 256) && tid == 128) {
    st_once(rec + kRecCount, sm[0][kRecCount]);
  } else if (tid < kNumAcc) {
    if (ACC == 0) {
      st_once(rec + kRecAcc + tid, (sm[0][kRecAcc + tid] + sm[1][kRecAcc + tid]) + (sm[2][kRecAcc + tid] + sm[3][kRecAcc + tid]));
    } else {
      constexpr int kW = kBufs * kWave * 16;  // floats between the staging areas of two waves
      float v;
      if (DVO_GRAM_BLOCKS) {
        auto rows = [&](const float *p) { return (p[0] + p[16]) + (p[32] + p[48]); };  // the four 16-lane rows of a wave
        auto waves = [&](const int e) { return (rows(stage + e) + rows(stage + kW + e)) + (rows(stage + 2 * kW + e) + rows(stage + 3 * kW + e)); };
        v = waves(e0);
        if (e1 >= 0) v += waves(e1);
      } else {
        v = (stage[e0] + stage[kW + e0]) + (stage[2 * kW + e0] + stage[3 * kW + e0]);
        if (e1 >= 0) v += (stage[e1] + stage[kW + e1]) + (stage[2 * kW + e1] + stage[3 * kW + e1]);
      }
      st_once(rec + kRecAcc + tid, v);
    }
  } else if (tid == 128) {
    // ordered combine of the four wave segments (see combine rule in k_finalize).  Everything is read first and the fold is
    // written without branches (an empty segment changes nothing, through selects): one round of LDS latency instead of
    // eight in the tail of every block
    unsigned CB[kWavesPerBlock];
    float FW[kWavesPerBlock], L0[kWavesPerBlock], L1[kWavesPerBlock], A0[kWavesPerBlock][3], A1[kWavesPerBlock][3];
#pragma unroll
    for (int wv = 0; wv < kWavesPerBlock; ++wv) {
      CB[wv] = f2u(sm[wv][kRecCount]), FW[wv] = sm[wv][kRecFirstW], L0[wv] = sm[wv][kRecLastR], L1[wv] = sm[wv][kRecLastR + 1];
#pragma unroll
      for (int i = 0; i < 3; ++i) A0[wv][i] = sm[wv][kRecS0 + i], A1[wv][i] = sm[wv][kRecS1 + i];
    }
    unsigned c = 0;
    float fw = 0.0f, l0 = 0.0f, l1 = 0.0f;
    float s0[3] = {0.0f, 0.0f, 0.0f}, s1[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int wv = 0; wv < kWavesPerBlock; ++wv) {
      st_once(rec + kRecWaveCnt + wv, u2f(CB[wv]));
      const bool ne = CB[wv] != 0;           // an empty segment is skipped
      const bool first = c == 0;             // nothing before it: its first weight is the combined segment's
      const bool flip = (c & 1u) != 0;       // b starts on the opposite parity of a
      const float bfw = FW[wv];
      // b's first pixel is a pair-second when b starts on an odd rank: it weights a's last residual
      const float r[3] = {l0 * l0, l0 * l1, l1 * l1};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        float x0 = flip ? A1[wv][i] : A0[wv][i];  // contribution if the combined segment starts even
        float x1 = flip ? A0[wv][i] : A1[wv][i];  // ... starts odd
        const float add = bfw * r[i];
        x0 = (!first && flip) ? x0 + add : x0;
        x1 = (!first && !flip) ? x1 + add : x1;
        s0[i] = ne ? s0[i] + x0 : s0[i];
        s1[i] = ne ? s1[i] + x1 : s1[i];
      }
      fw = (ne && first) ? bfw : fw;
      l0 = ne ? L0[wv] : l0, l1 = ne ? L1[wv] : l1;
      c += CB[wv];
    }
    st_once(rec + kRecCount, u2f(c));
    st_once(rec + kRecFirstW, fw);
    st_once(rec + kRecLastR, l0);
    st_once(rec + kRecLastR + 1, l1);
    for (int i = 0; i < 3; ++i) st_once(rec + kRecS0 + i, s0[i]), st_once(rec + kRecS1 + i, s1[i]);
    st_once(rec + 14, 0.0f), st_once(rec + 15, 0.0f);
#if defined(DVO_TRACE_BLOCKS) && defined(DVO_TRACE_TAIL)
    __hip_atomic_store(&trace_tail, trace_clock(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#endif
  }
}

// ------------------------------------------------------------------------------------------------------------------
// log-likelihood pass: sum over the first 50*floor(V/50) valid residuals of log(1 + 0.2 r^T P r)
// (computeCompleteDataLogLikelihood, dense_tracking_impl.cpp:406-425, incl. Q6).  Same segment geometry as the residual
// pass that wrote the residuals; {cut_seg, cut_local} locate global rank 50*floor(V/50).
// ------------------------------------------------------------------------------------------------------------------
// 1 + 0.2 q in double, one fused operation: the reference's expression (dense_tracking_impl.cpp:415) is contracted by its own
// build (-O3 -march=native, GNU contraction default), the oracle's portable build keeps the two roundings apart; the two differ by
// at most half an ulp of a double per term, far below the float the likelihood is returned as.  One fp64 operation less per pixel
// in a pass that is issue-bound on them.
__device__ __forceinline__ double ll_term(float q) { return __builtin_fma(0.2, (double)q, 1.0); }
// v_max_f32 without the canonicalising self-max the compiler puts in front of fmaxf's accumulator (q is never a signalling NaN)
__device__ __forceinline__ float max_raw(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

__device__ void loglik_pass(const TickItem &it, const LevelPairDesc &d, const int lb) {
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = threadIdx.x >> 6;
  // Merged blocks: likelihood block `lb` covers up to m residual blocks of the pass that filled the buffer, never across a chunk
  // boundary of the level's summation tree (ll_block_range); its wave w walks the `count` consecutive residual wave segments
  // from segment 4 first + w count on.  (A likelihood step is a tenth of a residual step's work: blocks as short as the
  // residual pass's are all prologue and hold a block slot for it.)  The geometry is a function of the level alone, so a lane's
  // running product -- and with it every log -- is cut at the same pixels whatever else the tick carries.
  int blk_first, blk_count;
  ll_block_range((int)it.ll_level_blocks, item_ll_merge_log2(it), lb, &blk_first, &blk_count);
  const int sub = item_ll_steps(it);                          // steps of one residual wave segment
  const int seg = blk_first * kWavesPerBlock + wave * blk_count;  // first residual wave segment of this wave
  const int steps = blk_count * sub;
  // The first chunk of residuals is requested BEFORE the prefix table is looked at (the table decides whether the segment counts
  // at all, but the addresses do not depend on it): one memory round trip less in the dependent chain every block starts with.
  constexpr int kLlChunk = 16;
  v2f cur[kLlChunk], nxt[kLlChunk];
  const DVO_GLOBAL v2f *src = (const DVO_GLOBAL v2f *)((it.flags & kItemLlBuf) ? d.res[1] : d.res[0]) + seg * (kStepPx * sub) + lane;
  auto load_chunk = [&](v2f(&dst)[kLlChunk], const int first) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kLlChunk; ++k)
      if (first + k < steps) dst[k] = ld_once(src + (first + k) * kWave);
  };
  load_chunk(cur, 0);
  // valid pixels of this band that precede the segment (written by k_finalize of the residual pass that filled the buffer)
  const int seg_before =
      steps > 0 ? ((const DVO_GLOBAL int *)((it.flags & kItemLlBuf) ? d.seg_prefix[1] : d.seg_prefix[0]))[seg] : 0;
  const int cut_rank = it.ll_cut_rank;
  const float P0 = it.P[0], P1 = it.P[1], P2 = it.P[2], P3 = it.P[3];
  const unsigned long long below = (1ull << lane) - 1ull;
  double total = 0.0;
  // The largest Mahalanobis distance among the residuals that count: the reference multiplies 50 consecutive terms
  // 1 + 0.2 q in a double before it takes a log (dense_tracking_impl.cpp:413-419), and that product overflows -- likelihood
  // -inf, iteration rejected -- when 50 consecutive q are all above ~7e6 (noise-free synthetic depth; never sensor data).
  // Here a log is taken before the running product can leave the double range, so nothing overflows; the host is told the largest q of the pass and, only if one
  // group of 50 COULD have overflowed, asks k_ll_overflow for the exact answer (dvo_tracker.cpp: ll_overflowed).
  float qmax = 0.0f;
  if (steps > 0 && seg_before < cut_rank) {
    int run_count = seg_before;
    // four steps (256 pixels) per trip; the terms 1 + 0.2 r^T P r >= 1 of a lane are multiplied up in a double and a log
    // is taken of the product, like the reference takes one log per 50 residuals (dense_tracking_impl.cpp:415-419) -- here
    // whenever the product has grown past 1e150 (checked once per trip) and at the end of the segment: the fp64 log is ninety
    // instructions, and one per sixteen terms was two fifths of this pass's issue time
    double prod = 1.0;
    const bool all_below_cut = seg_before + steps * kWave <= cut_rank;  // wave uniform: every pixel of the segment counts
    // The residuals are fetched kLlChunk steps at a time and one chunk ahead of the arithmetic: sixteen 8-byte loads per lane in
    // flight while the previous sixteen steps are worked through.  (Until round 4 a trip loaded its four steps and then used them:
    // a block of the likelihood pass spent its life waiting for memory -- 24 us for 32 steps, more than a residual block's 17 us
    // for a tenth of the instructions -- and the pass held a quarter of the GPU's block slots: scripts/block_trace.py.)  The
    // arithmetic, and the order it is done in, are unchanged: trips of four steps, the product checked once per trip.
    for (int c0 = 0; c0 < steps; c0 += kLlChunk) {
      if (c0 + kLlChunk < steps) load_chunk(nxt, c0 + kLlChunk);
#pragma unroll
      for (int t = 0; t < kLlChunk; t += 4) {
        if (c0 + t >= steps) break;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if (c0 + t + k >= steps) break;
          const v2f r = cur[t + k];
          const bool valid = r.x == r.x;
          if (all_below_cut) {  // only the segment(s) around rank 50 * floor(V / 50) need ranks: Q6 drops at most 49 residuals
            if (valid) {
              const float t0 = r.x * P0 + r.y * P1;
              const float t1 = r.x * P2 + r.y * P3;
              const float q = t0 * r.x + t1 * r.y;
              prod *= ll_term(q);
              qmax = max_raw(qmax, q);
            }
            continue;
          }
          const unsigned long long b = __ballot(valid);
          const int rank = run_count + __popcll(b & below);
          if (valid && rank < cut_rank) {
            const float t0 = r.x * P0 + r.y * P1;
            const float t1 = r.x * P2 + r.y * P3;
            const float q = t0 * r.x + t1 * r.y;
            prod *= ll_term(q);
            qmax = max_raw(qmax, q);
          }
          run_count += __popcll(b);
        }
        // a log only when the running product gets large: a term is at most 1 + 0.2 * FLT_MAX < 7e37, so four more of them on top
        // of 1e150 stay below the double range; with ordinary residuals (terms of 1 .. 20) a lane takes one log per wave segment
        if (prod > 1e150) {
          total += log(prod);
          prod = 1.0;
        }
      }
#pragma unroll
      for (int k = 0; k < kLlChunk; ++k) cur[k] = nxt[k];
    }
    if (prod != 1.0) total += log(prod);
  }
  total = wave_sum_double(total);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) qmax = __builtin_fmaxf(qmax, __shfl_xor(qmax, m, 64));
  __shared__ double smd[kWavesPerBlock];
  __shared__ float smq[kWavesPerBlock];
  if (lane == 0) smd[wave] = total, smq[wave] = qmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    ((DVO_GLOBAL double *)d.ll_partials)[lb] = (smd[0] + smd[1]) + (smd[2] + smd[3]);
    ((DVO_GLOBAL float *)d.ll_qmax)[lb] = __builtin_fmaxf(__builtin_fmaxf(smq[0], smq[1]), __builtin_fmaxf(smq[2], smq[3]));
  }
}

// The exact answer to "did the reference's 50-term likelihood product overflow?" for one residual buffer, asked only when the
// pass above saw a Mahalanobis distance large enough to make it possible.  A block is ONE wave and owns the groups of fifty
// consecutive valid residuals (in rank order) that START inside its chunk of `segs_per_block` wave segments of the residual
// pass: the prefix table gives the rank of the chunk's first valid pixel, the wave skips what is left of the previous chunk's
// last group, walks on in scan order -- past the end of its chunk until its last group is complete -- compacts the terms
// 1 + 0.2 q into LDS in rank order, and lane g multiplies group g's fifty terms one after the other in a double: the
// reference's own loop (error_acc *= ..., dense_tracking_impl.cpp:415-417), so the decision is the reference's bit for bit.
constexpr int kOvfGroups = 64, kOvfWindow = kOvfGroups * 50;
__global__ __launch_bounds__(kWave) void k_ll_overflow(const float2 *__restrict__ res, const int *__restrict__ seg_prefix, int seg_first,
                                                       int n_segs, int segs_per_block, int seg_px, int rank_offset, int n_px,
                                                       int cut_rank, int rank_end, float P0, float P1, float P2, float P3,
                                                       unsigned *__restrict__ result_host) {
  __shared__ double terms[kOvfWindow + kWave];
  const int lane = threadIdx.x;
  const unsigned long long below = (1ull << lane) - 1ull;
  const int s0 = seg_first + (int)blockIdx.x * segs_per_block;      // first wave segment of the chunk
  const int s1 = s0 + segs_per_block < seg_first + n_segs ? s0 + segs_per_block : seg_first + n_segs;
  const int a = rank_offset + seg_prefix[s0];                        // global rank of the chunk's first valid pixel
  // rank of the first valid pixel BEHIND the chunk (only the chunk's own segments are known to hold this pass's residuals)
  // rank_end >= 0: the band is CLOSED -- the residuals behind it live on another GPU -- and rank_end is the rank of the first
  // valid pixel behind it: the band's last chunk then stops at the last group that ends inside the band (the group that
  // straddles the edge is settled by the host from the ranks' edge records, dvo_sharded.cpp: sharded_overflow)
  const bool last_chunk = s1 >= seg_first + n_segs;
  const int e = !last_chunk ? rank_offset + seg_prefix[s1] : (rank_end >= 0 ? rank_end : 0x7fffffff);
  const int first = a + (50 - a % 50) % 50;                          // first group that starts in the chunk
  int stop = e >= cut_rank ? cut_rank                                // (cut_rank is a multiple of 50)
             : (last_chunk && rank_end >= 0) ? e - e % 50            // closed band: complete groups only
                                             : e + (50 - e % 50) % 50;  // ... else the end of the group that straddles the chunk's end
  // A closed band: NO chunk may follow a group past the band's last valid pixel -- a chunk that is not the band's last one can
  // still hold the start of the group that straddles the band edge when fewer than fifty valid pixels lie behind it (a depth
  // hole at the band edge); the residuals behind the edge are another GPU's, this rank's copy of them is stale
  int px_end = n_px;
  if (rank_end >= 0) {
    const int closed = rank_end - rank_end % 50;
    stop = stop < closed ? stop : closed;
    px_end = (seg_first + n_segs) * seg_px;
  }
  if (first >= stop) return;
  int run = a, base = first;  // rank of the next valid pixel; rank of terms[0]
  bool overflow = false;
  auto flush = [&](int n_groups) {  // lanes 0 .. n_groups - 1 multiply one group each
    __syncthreads();
    if (lane < n_groups) {
      double acc = 1.0;
      for (int i = 0; i < 50; ++i) acc *= terms[lane * 50 + i];
      overflow = overflow || !(acc <= 1.7976931348623157e308);
    }
    __syncthreads();
  };
  for (int i0 = s0 * seg_px; i0 < px_end && run < stop; i0 += kWave) {
    const float2 r = res[i0 + lane];  // (the buffer is padded to whole wave segments)
    const bool valid = r.x == r.x;
    const unsigned long long b = __ballot(valid);
    const int rank = run + __popcll(b & below);
    if (valid && rank >= first && rank < stop) {
      const float t0 = r.x * P0 + r.y * P1;
      const float t1 = r.x * P2 + r.y * P3;
      const float q = t0 * r.x + t1 * r.y;
      terms[rank - base] = 1.0 + 0.2 * (double)q;
    }
    run += __popcll(b);
    const int have = (run < stop ? run : stop) - base;
    if (have >= kOvfWindow) {
      flush(kOvfGroups);
      const double t = terms[kOvfWindow + lane];  // at most 63 terms of the next window: move them to the front
      __syncthreads();
      if (lane < have - kOvfWindow) terms[lane] = t;
      __syncthreads();
      base += kOvfWindow;
    }
  }
  const int left = (run < stop ? run : stop) - base;
  if (left >= 50) flush(left / 50);  // (a last group cut short by the end of the buffer cannot exist: cut_rank <= V)
  const unsigned long long any = __ballot(overflow);
  if (lane == 0 && any) __hip_atomic_store(result_host, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// Copy the descriptors into registers once, through the constant address space (scalar loads).  Read through plain global
// references their fields would be re-loaded with vector loads + s_waitcnt vmcnt(0) at every use inside the pixel loop,
// because the residual stores might alias them: ten dependent L2 round trips per 64 pixels.
#define DVO_CONST __attribute__((address_space(4)))
__device__ __forceinline__ LevelPairDesc load_desc(const TickItem &it) {
  const DVO_CONST RefLevelDesc *r = (const DVO_CONST RefLevelDesc *)it.ref;
  const DVO_CONST CurLevelDesc *c = (const DVO_CONST CurLevelDesc *)it.cur;
  const DVO_CONST SlotDesc *s = (const DVO_CONST SlotDesc *)it.slot;
  LevelPairDesc d;
  d.r_zsel = r->r_zsel, d.r_i = r->r_i, d.r_ix = r->r_ix, d.r_iy = r->r_iy;
  d.tx = r->tx, d.ty = r->ty;
  d.c_a = c->c_a, d.c_b = c->c_b;
  d.w = c->w, d.h = c->h;
#pragma unroll
  for (int i = 0; i < 6; ++i) d.wc[i] = c->wc[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) d.wr[i] = c->wr[i];
  d.ub_x = c->ub_x, d.ub_y = c->ub_y;
  d.res[0] = s->res[0], d.res[1] = s->res[1];
  d.records = s->records, d.ll_partials = s->ll_partials, d.ll_qmax = s->ll_qmax;
  d.seg_prefix[0] = s->seg_prefix[0], d.seg_prefix[1] = s->seg_prefix[1];
  return d;
}

template <int ACC, int RCP>
__device__ __forceinline__ void tick_body(const TickItem &it, const RcpTable &rcp, const int bx) {
  const int rb = it.res_blocks;
  if (bx >= rb + it.ll_blocks) return;
#ifdef DVO_TRACE_BLOCKS
  const unsigned long long trace_t0 = trace_clock();
  // (the record's slot is taken NOW: the atomic's round trip, ~0.6 us under load, must not sit in front of the end stamp -- it did
  //  until the end of round 4, and every block looked that much longer)
  unsigned trace_slot = 0;
  if (threadIdx.x == 0) trace_first = 0, trace_tail = 0, trace_slot = atomicAdd(&g_trace_n, 1u);
#endif
  LevelPairDesc d = load_desc(it);
#ifdef DVO_TRACE_DESC  // (a variant of the trace: the "first step" stamp is taken when the descriptors have arrived instead)
  if (threadIdx.x == 0) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    DVO_KEEP(d.w);
    trace_first = trace_clock();
  }
#endif
  d.rcp = rcp;
  d.rcp_lds = nullptr;
  d.dbg_w = RCP ? ((const DVO_CONST SlotDesc *)it.slot)->dbg_w : nullptr;
  if (bx < rb)
    residual_pass<ACC, RCP>(it, d, it.res_first + xcd_contiguous_block(bx, rb));
  else
    loglik_pass(it, d, (int)it.ll_first + (bx - rb));
#ifdef DVO_TRACE_BLOCKS
  if (threadIdx.x == 0) {
    const unsigned long long trace_t1 = trace_clock();
    const unsigned slot = trace_slot;
    if (slot < kTraceCapacity) {
      unsigned hw, xcc;
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
      asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
      BlockTrace t;
      t.t0 = trace_t0, t.t_first = trace_first, t.t_end = trace_t1;
#ifdef DVO_TRACE_TAIL  // (the block's other tail: spin until thread 128 has stamped, at most ~20 us; t_first carries its stamp)
      if (bx < rb) {
        const unsigned long long t_spin = trace_clock();
        unsigned long long tail = 0;
        while ((tail = __hip_atomic_load(&trace_tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) == 0 && trace_clock() - t_spin < 2000) {}
        t.t_first = tail;
      }
#endif
      t.info = (unsigned)(bx < rb ? (it.steps_log2 & 15) : (it.steps_log2 >> 4)) | (bx < rb ? 0u : 16u) | ((unsigned)(d.w / 8) << 8) |
               ((unsigned)(bx < rb ? rb : it.ll_blocks) << 16);
      t.hw = (hw & 0x0fffffffu) | (xcc << 28);
      g_trace[slot] = t;
    }
  }
#endif
}

// Which of its owner's blocks is block `block` of the grid?  idx: the item whose range of block groups holds it (a set's first
// item when the set is dispatched interleaved: TickArgs::set_size).  Returns the item and leaves its block in bx.  Shared with
// the host's restatement (tick_args_locate).
template <class Args>
__host__ __device__ __forceinline__ int tick_place(const Args &args, int idx, int pos, const unsigned block, int &bx) {
  if constexpr (Args::kSets) {
    // (compact == 2: a launch-wide flag that is there with the kernel's first arguments, so that a launch without interleaved
    //  sets does not put set_size's load in front of everything that depends on idx -- measured: 1.3 % of the batch)
    if (args.compact > 1) {
      const unsigned m = args.set_size[idx];
      if (m > 1) {
        const unsigned q = (unsigned)(((unsigned long long)(unsigned)pos * args.set_inv[idx]) >> 32);  // pos / m
        idx += pos - (int)(q * m);
        pos = (int)q;
      }
    }
  }
  const int rot = pos < (int)(args.items[idx].res_blocks >> 3) ? args.xcd_rot[idx] : args.tail_rot[idx];
  bx = (pos << 3) | (int)((block + (unsigned)rot) & 7u);
  return idx;
}

// Which item owns this block, and which of the item's blocks is it?  Two-dimensional grid: (block, item).  One-dimensional
// ("compact") grid: lanes 0 .. n_items look at the items' first block groups; the owner is the last item that starts at or
// before this block's group (every wave finds the same one).
template <class Args>
__device__ __forceinline__ int tick_locate(const Args &args, int &bx, const unsigned block = blockIdx.x) {
  constexpr int kSlots = (int)(sizeof(args.group_first) / sizeof(args.group_first[0]));
  if (!args.compact) return tick_place(args, (int)blockIdx.y, (int)(block >> 3), block, bx);
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned g = block >> 3;
  const unsigned first = lane <= args.n_items ? (unsigned)args.group_first[lane < kSlots ? lane : 0] : 0xFFFFFFFFu;
  const int idx = __builtin_amdgcn_readfirstlane(__popcll(__ballot(first <= g)) - 1);
  return tick_place(args, idx, (int)g - (int)args.group_first[idx], block, bx);
}

// ACC 1 (default): Gram matrix on the matrix pipe, 4 waves per SIMD.  ACC 0 (DVO_AMD_ACCUM=valu): 87 fp32 registers per lane,
// 2 waves per SIMD -- kept as the cross-check of the summation (tests/test_gpu_parity.py runs the parity suite's criterion under it).
template <int ACC, int RCP>
__global__ __launch_bounds__(kBlockThreads, ACC == 0 ? 2 : 4) void k_tick(const TickArgs args) {
  int bx;
  const int idx = tick_locate(args, bx);
  tick_body<ACC, RCP>(args.items[idx], args.rcp, bx);
}

// the same kernel behind the small argument block of a tick of at most kMaxSmallItems pairs
template <int RCP>
__global__ __launch_bounds__(kBlockThreads, 4) void k_tick_small(const TickArgsSmall args) {
  int bx;
  const int idx = tick_locate(args, bx);
  tick_body<1, RCP>(args.items[idx], args.rcp, bx);
}

// ---- Q7 in the host-rcpps mode (dense_tracking_impl.cpp:702-706; Q7Rec in dvo_types.h) -------------------------------------------
// One wave per residual pass of a tick launch, after k_tick and before k_finalize on the same stream: V from the pass's block
// records, the last V mod 4 valid pixels from the per-wave counts and the spilled residuals (walked backwards), then those <= 3
// pixels once more through the residual pass's own functions -- lane j takes tail pixel j -- for their Jacobians, and what
// (w_exact - w_table) adds to the pair sums (Q5: an odd rank weights its partner's residual; the tail starts on a multiple of
// four, so the partner is in the tail) and to the 87 moments, in double.  Costs one small dispatch per tick, in this mode only.
template <class Args>
__device__ __forceinline__ void q7_tail_wave(const Args &args) {
  const TickItem &it = args.items[blockIdx.x];
  const int lane = threadIdx.x;
  LevelPairDesc d = load_desc(it);
  d.rcp = args.rcp;
  d.rcp_lds = nullptr, d.dbg_w = nullptr;
  DVO_GLOBAL Q7Rec *const rec = (DVO_GLOBAL Q7Rec *)((DVO_GLOBAL char *)d.ll_partials + 256u * (unsigned)args.q7_off256);
  const gcf recs = (gcf)d.records;
  const int nb = it.res_blocks, steps = item_res_steps(it), seg_px = kStepPx * steps;
  int v = 0;
  for (int b = lane; b < nb; b += kWave) v += (int)f2u(recs[(size_t)b * kRecStride + kRecCount]);
  for (int o = kWave / 2; o; o >>= 1) v += __shfl_xor(v, o);
  const int n_tail = (it.flags & kItemUnitWeights) ? 0 : (v & 3);
  __shared__ double sh_delta[3][3 + kNumAcc];
  __shared__ int sh_idx[3];
  __shared__ float sh_r0[3], sh_r1[3];
  if (lane < 3) {
    sh_idx[lane] = 0, sh_r0[lane] = sh_r1[lane] = 0.0f;
    for (int i = 0; i < 3 + kNumAcc; ++i) sh_delta[lane][i] = 0.0;
  }
  __syncthreads();
  int found = 0;  // wave uniform; tail pixels are found last first
  if (n_tail) {
    const DVO_GLOBAL v2f *const res = (const DVO_GLOBAL v2f *)((it.flags & kItemResBuf) ? d.res[1] : d.res[0]);
    for (int sg = nb * kWavesPerBlock - 1; sg >= 0 && found < n_tail; --sg) {
      const int c = __builtin_amdgcn_readfirstlane((int)f2u(recs[(size_t)(sg >> 2) * kRecStride + kRecWaveCnt + (sg & 3)]));
      if (c == 0) continue;
      for (int st = steps - 1; st >= 0 && found < n_tail; --st) {
        const int first = sg * seg_px + st * kStepPx;
        const v2f r = res[first + lane];
        unsigned long long m = __ballot(r.x == r.x);  // NaN marks an invalid pixel
        while (m && found < n_tail) {
          const int hi = 63 - __builtin_clzll(m);
          const float r0 = __shfl(r.x, hi), r1 = __shfl(r.y, hi);
          if (lane == 0) sh_idx[found] = first + hi, sh_r0[found] = r0, sh_r1[found] = r1;
          m &= ~(1ull << hi);
          ++found;
        }
      }
    }
    __syncthreads();
  }
  const bool mine = lane < n_tail && found == n_tail;
  float w_table = 0.0f, w_exact = 0.0f;
  bool equal = true;
  int my_idx = 0;
  if (n_tail && found == n_tail) {  // (wave uniform; every lane walks a real pixel, lanes past the tail walk tail pixel 0 for nothing)
    const int j = lane < n_tail ? lane : 0;  // ascending rank: tail pixel j was found (n_tail - 1 - j)-th
    const int k = n_tail - 1 - j;
    const unsigned idx = (unsigned)sh_idx[k];
    my_idx = (int)idx;
    float z = ((gcf)d.r_zsel)[idx], ri = ((gcf)d.r_i)[idx], rix = ((gcf)d.r_ix)[idx], riy = ((gcf)d.r_iy)[idx];
    float x = ((gcf)d.tx)[idx] * z, y = ((gcf)d.ty)[idx] * z;
    float kt[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) kt[i] = it.kt[i];
    DVO_OPAQUE(x); DVO_OPAQUE(y); DVO_OPAQUE(z); DVO_OPAQUE(ri); DVO_OPAQUE(rix); DVO_OPAQUE(riy);
    round_toward_zero();
    DVO_OPAQUE(x); DVO_OPAQUE(y); DVO_OPAQUE(z); DVO_OPAQUE(ri); DVO_OPAQUE(rix); DVO_OPAQUE(riy);
    float r0, r1, e2, e3, e4, e5;
    bool ok;
    {
      const Proj p = project_pixel_rtz<1>(kt, d, x, y, z);
      const Gathered g = gather_pixel(d, p.base);
      finish_pixel_rtz<true>(d, p, g, z, ri, rix, riy, r0, r1, e2, e3, e4, e5, ok);
    }
    DVO_OPAQUE(r0); DVO_OPAQUE(r1); DVO_OPAQUE(e2); DVO_OPAQUE(e3); DVO_OPAQUE(e4); DVO_OPAQUE(e5);
    DVO_OPAQUE(x); DVO_OPAQUE(y); DVO_OPAQUE(z);
    round_to_nearest();
    DVO_OPAQUE(r0); DVO_OPAQUE(r1); DVO_OPAQUE(e2); DVO_OPAQUE(e3); DVO_OPAQUE(e4); DVO_OPAQUE(e5);
    DVO_OPAQUE(x); DVO_OPAQUE(y); DVO_OPAQUE(z);
    equal = ok && f2u(r0) == f2u(sh_r0[k]) && f2u(r1) == f2u(sh_r1[k]);
    // the two weights (the distance as computeWeightsSse / computeWeight form it: product by product)
    const float t0 = r0 * it.P[0] + r1 * it.P[1];
    const float t1 = r0 * it.P[2] + r1 * it.P[3];
    const float dd = t0 * r0 + t1 * r1;
    w_table = 7.0f * rcp_host_table(5.0f + dd, d.rcp);
    w_exact = (float)((2.0 + 5.0f) / (5.0f + dd));  // :643, the division in double
    const double dw = mine ? (double)w_exact - (double)w_table : 0.0;
    // Jacobian rows as the residual pass forms them (without the sqrt(w) of the staged form)
    const float iz = __builtin_amdgcn_rcpf(z);
    const float iz2 = iz * iz;
    const float j02 = -x * iz2, j12 = -y * iz2;
    const float j03 = j02 * y, j13 = __builtin_fmaf(j12, y, -1.0f);
    const float j04 = __builtin_fmaf(-j02, x, 1.0f), j14 = -j03;
    const float j05 = -y * iz, j15 = x * iz;
    float Ja[6], Jb[6];
    Ja[0] = e2 * iz;
    Ja[1] = e3 * iz;
    Ja[2] = __builtin_fmaf(e2, j02, e3 * j12);
    Ja[3] = __builtin_fmaf(e2, j03, e3 * j13);
    Ja[4] = __builtin_fmaf(e2, j04, e3 * j14);
    Ja[5] = __builtin_fmaf(e2, j05, e3 * j15);
    Jb[0] = e4 * iz;
    Jb[1] = e5 * iz;
    Jb[2] = __builtin_fmaf(e4, j02, __builtin_fmaf(e5, j12, -1.0f));
    Jb[3] = __builtin_fmaf(e4, j03, __builtin_fmaf(e5, j13, -y));
    Jb[4] = __builtin_fmaf(e4, j04, __builtin_fmaf(e5, j14, x));
    Jb[5] = __builtin_fmaf(e4, j05, e5 * j15);
    if (lane < 3) {
      double *o = sh_delta[lane];
      // pair sums: an even rank weights its own residual, an odd one its partner's (tail pixel 0: the tail starts on a multiple of 4)
      const float a0 = (j & 1) ? sh_r0[n_tail - 1] : r0, a1 = (j & 1) ? sh_r1[n_tail - 1] : r1;
      o[0] = dw * (double)(a0 * a0), o[1] = dw * (double)(a0 * a1), o[2] = dw * (double)(a1 * a1);
      double *acc = o + 3;
      int t = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int c = i; c < 6; ++c, ++t) {
          acc[kAccAA + t] = dw * ((double)Ja[i] * (double)Ja[c]);
          acc[kAccAB + t] = dw * ((double)Ja[i] * (double)Jb[c] + (double)Jb[i] * (double)Ja[c]);
          acc[kAccBB + t] = dw * ((double)Jb[i] * (double)Jb[c]);
        }
        acc[kAccAR0 + i] = dw * ((double)Ja[i] * (double)r0);
        acc[kAccAR1 + i] = dw * ((double)Ja[i] * (double)r1);
        acc[kAccBR0 + i] = dw * ((double)Jb[i] * (double)r0);
        acc[kAccBR1 + i] = dw * ((double)Jb[i] * (double)r1);
      }
    }
  }
  __syncthreads();
  for (int i = lane; i < 3 + kNumAcc; i += kWave) {
    const double sum = (sh_delta[0][i] + sh_delta[1][i]) + sh_delta[2][i];
    if (i < 3) rec->S[i] = sum; else rec->acc[i - 3] = sum;
  }
  const unsigned long long all_equal = __ballot(!mine || equal);
  if (lane < 3) {
    rec->idx[lane] = mine ? my_idx : -1;
    rec->w_table[lane] = mine ? w_table : 0.0f;
    rec->w_exact[lane] = mine ? w_exact : 0.0f;
  }
  if (lane == 0) {
    rec->n_tail = found == n_tail ? n_tail : -1;  // (-1: the counts and the residual buffer disagree -- cannot happen)
    rec->valid = v;
    rec->recomputed_equal = all_equal == ~0ull ? 1 : 0;
  }
}
__global__ __launch_bounds__(kWave) void k_q7_tail(const Q7Args args) { q7_tail_wave(args); }
__global__ __launch_bounds__(kWave) void k_q7_tail_small(const Q7ArgsSmall args) { q7_tail_wave(args); }

__global__ void k_rcp_table_probe(const RcpTable rcp, const float *__restrict__ in, float *__restrict__ out, int n) {
  __shared__ unsigned nib[kRcpNibbleWordsMax];
  if (rcp.nibbles) {
    for (int i = threadIdx.x; i < ((1 << (23 - rcp.shift)) >> 3); i += blockDim.x) nib[i] = rcp.nibbles[i];
    __syncthreads();
  }
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = rcp.nibbles ? rcp_host_nibbles<false>(in[i], nib, rcp.shift, rcp.unit) : rcp_host_table(in[i], rcp);
}
// v_rcp_f32 of every cell midpoint under both rounding modes the residual pass uses it in (the host builds the corrections of the
// nibble form from the round-to-nearest column and refuses the form if the columns differ)
__global__ void k_rcp_midpoint_probe(int k, unsigned *__restrict__ out_rn, unsigned *__restrict__ out_rtz) {
  const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << k)) return;
  unsigned cell = i;
  asm volatile("" : "+v"(cell));
  const unsigned a = rcp_midpoint_bits(cell, 23 - k);
  unsigned keep = a;
  asm volatile("" : "+v"(keep));
  round_toward_zero();
  asm volatile("" : "+v"(cell));
  unsigned b = rcp_midpoint_bits(cell, 23 - k);
  asm volatile("" : "+v"(b));
  round_to_nearest();
  out_rn[i] = keep, out_rtz[i] = b;
}

// DVO_AMD_LAUNCH_LOCK=1: a process-wide mutex around every kernel launch.  Only for profiled multi-thread runs: rocprofv3's
// queue interceptor reads past the end of an AQL ring when two host threads publish packets to one hardware queue across
// the ring's wrap (profiles/r03_rocprofv3_sigsegv_root_cause.md); under the lock every doorbell finds exactly one packet.
static std::mutex g_launch_mu;
static bool launch_lock_enabled() {  // (function-local statics: initialised once, thread-safe)
  static const bool on = [] {
    const char *e = getenv("DVO_AMD_LAUNCH_LOCK");
    return e && e[0] == '1';
  }();
  return on;
}
struct LaunchGuard {
  bool held;
  LaunchGuard() {
    held = launch_lock_enabled();
    if (held) g_launch_mu.lock();
  }
  ~LaunchGuard() {
    if (held) g_launch_mu.unlock();
  }
};

// DVO_AMD_ACCUM=valu: 87 register accumulators; default: the Gram matrix on the matrix pipe
int acc_mode() {
  static const int m = [] {
    const char *a = getenv("DVO_AMD_ACCUM");
    return (a && (a[0] == 'v' || a[0] == 'V' || a[0] == '0')) ? 0 : 1;
  }();
  return m;
}

typedef void (*TickKernel)(const TickArgs);
// (the host-rcpps mode exists for the default accumulator only)
static TickKernel pick_tick_kernel(const RcpTable &rcp) {
  return rcp.nibbles ? k_tick<1, 2> : rcp.table ? k_tick<1, 1> : acc_mode() == 0 ? k_tick<0, 0> : k_tick<1, 0>;
}

// A tick's items are at different pyramid levels: the two-dimensional grid (blocks of the largest item x items) launches
// mostly blocks that return at once, and the dispatcher starts only ~4 of them per nanosecond.  When more than half of the
// grid would be such blocks the launch goes out one-dimensional with every item's blocks back to back.
//
// Where an item's blocks run (TickArgs::xcd_rot, tail_rot, set_size).  Loads are in units of ~0.1 us of block life as the block
// trace measures it (a residual block: 3.3 us + 2.1 us per step; a likelihood block about half of that).
//   share 0: greedy over the items in launch order, one rotation per item, the one that leaves the smallest maximum XCD load.
//   share 1: the same greedy over SETS -- runs of neighbours in launch order that read the same reference level with the same
//     geometry (tick_items_order puts them next to each other) -- with one rotation for all members, so that XCD x works on
//     the same eighth of every member's segments and the members meet in its L2.  A set's remainder blocks repeat once per
//     member; where the sets' rotations leave the XCDs' loads more than 2 % of their mean apart, all full groups of the
//     launch stay unrotated and the greedy rotates every item's tail (partial residual group + likelihood blocks) instead.
//   share 2: ... and each set of the compact grid is dispatched interleaved (TickArgs::set_size).
// Sets of one item give the layout of share 0 exactly; so does the two-dimensional grid under every value.
static bool same_set(const TickItem &a, const TickItem &b) {
  return a.res_blocks > 0 && a.ref == b.ref && a.res_blocks == b.res_blocks && a.res_first == b.res_first &&
         (a.steps_log2 & 15) == (b.steps_log2 & 15);
}
static int layout_tail_mode() {  // DVO_AMD_SHARE_TAIL=0 / 1: never / always rotate the tails alone (tuning; default: the 2 % rule)
  static const int m = [] {
    const char *e = getenv("DVO_AMD_SHARE_TAIL");
    return e ? (e[0] == '0' ? 0 : 1) : 2;
  }();
  return m;
}
template <class Args>
static int tick_args_layout_impl(Args &args, int max_blocks, int share) {
  constexpr int kSlots = (int)(sizeof(args.group_first) / sizeof(args.group_first[0]));
  constexpr int kRots = (int)(sizeof(args.xcd_rot) / sizeof(args.xcd_rot[0]));
  const int n = args.n_items;
  if constexpr (!Args::kSets) share = 0;
  static const bool rotate = [] {
    const char *e = getenv("DVO_AMD_XCD_ROTATE");
    return !(e && e[0] == '0');
  }();
  // the sets: set_len[i] = members of the set that starts at item i (0: item i belongs to an earlier item's set)
  int set_len[kRots] = {};
  bool any_set = false;
  for (int i = 0; i < n;) {
    int j = i + 1;
    while (share > 0 && j < n && same_set(args.items[i], args.items[j])) ++j;
    set_len[i] = j - i;
    any_set = any_set || j - i > 1;
    i = j;
  }
  // what item i puts on the XCD that runs its blocks of phase f (blocks f, f + 8, ... before the rotation)
  long long phase[kRots][8];
  for (int i = 0; i < n; ++i) {
    const TickItem &it = args.items[i];
    const int rb = it.res_blocks, lb = it.ll_blocks;
    const long long w_res = 33 + 21 * item_res_steps(it), w_ll = 40 + 7 * item_ll_steps(it);
    for (int f = 0; f < 8; ++f) {
      const int n_res = (rb >> 3) + (f < (rb & 7) ? 1 : 0);
      const int all = ((rb + lb) >> 3) + (f < ((rb + lb) & 7) ? 1 : 0);
      phase[i][f] = w_res * n_res + w_ll * (all - n_res);
    }
  }
  long long load[8];
  // greedy over runs of items [i, i + len(i)): XCD x does the blocks of phase (x + rot) & 7 of every item of the run
  auto balance = [&](bool by_set, uint8_t *rot_out) {
    for (int x = 0; x < 8; ++x) load[x] = 0;
    for (int i = 0; i < n;) {
      const int len = by_set ? set_len[i] : 1;
      long long ph[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      for (int k = i; k < i + len; ++k)
        for (int f = 0; f < 8; ++f) ph[f] += phase[k][f];
      int best = 0;
      long long best_max = -1;
      for (int rot = 0; rotate && rot < 8; ++rot) {
        long long mx = 0;
        for (int x = 0; x < 8; ++x) mx = std::max(mx, load[x] + ph[(x + rot) & 7]);
        if (best_max < 0 || mx < best_max) best_max = mx, best = rot;
      }
      for (int k = i; k < i + len; ++k) rot_out[k] = (uint8_t)best;
      for (int x = 0; x < 8; ++x) load[x] += ph[(x + best) & 7];
      i += len;
    }
  };
  balance(true, args.xcd_rot);
  for (int i = 0; i < n; ++i) args.tail_rot[i] = args.xcd_rot[i];
  if (any_set && rotate) {
    long long lo = load[0], hi = load[0], sum = 0;
    for (int x = 0; x < 8; ++x) lo = std::min(lo, load[x]), hi = std::max(hi, load[x]), sum += load[x];
    const int tail_mode = layout_tail_mode();
    if (tail_mode == 1 || (tail_mode == 2 && (hi - lo) * 8 * 50 > sum)) {  // more than 2 % of the mean apart
      balance(false, args.tail_rot);
      for (int i = 0; i < n; ++i) args.xcd_rot[i] = 0;
    }
  }
  for (int i = n; i < kRots; ++i) args.xcd_rot[i] = args.tail_rot[i] = 0;

  const bool interleave = share > 1 && any_set;
  unsigned groups = 0;
  auto item_groups = [&](int i) { return ((unsigned)args.items[i].res_blocks + args.items[i].ll_blocks + 7u) >> 3; };
  for (int i = 0; i < n;) {
    const int len = interleave ? set_len[i] : 1;
    unsigned widest = 0;
    for (int k = i; k < i + len; ++k) widest = std::max(widest, item_groups(k));
    args.group_first[i] = (uint16_t)groups;
    groups += (unsigned)len * widest;
    for (int k = i + 1; k < i + len; ++k) args.group_first[k] = (uint16_t)groups;
    if constexpr (Args::kSets) {
      for (int k = i; k < i + len; ++k) args.set_size[k] = 1, args.set_inv[k] = 0;
      if (len > 1) args.set_size[i] = (uint8_t)len, args.set_inv[i] = (uint32_t)(0xFFFFFFFFull / (unsigned)len + 1ull);
    }
    i += len;
  }
  for (int i = n; i < kSlots; ++i) args.group_first[i] = (uint16_t)groups;
  if constexpr (Args::kSets)
    for (int i = n; i < kRots; ++i) args.set_size[i] = 1;
  const long long grid2d = (long long)((max_blocks + 7) & ~7) * args.n_items;
  static const int mode = [] {  // DVO_AMD_COMPACT_GRID=0 / 1 forces a layout (tuning)
    const char *e = getenv("DVO_AMD_COMPACT_GRID");
    return e ? (e[0] == '0' ? 0 : 1) : 2;
  }();
  // (the surplus blocks of an interleaved set are few -- its members differ in their likelihood blocks only -- and are not
  //  counted: the choice between the grids is the one share 0 makes)
  unsigned own_groups = 0;
  for (int i = 0; i < n; ++i) own_groups += item_groups(i);
  args.compact = groups > 0 && groups < 65536 && (mode == 1 || (mode == 2 && 2ll * 8 * own_groups < grid2d)) ? (interleave ? 2 : 1) : 0;
  if (!args.compact && share > 0) return tick_args_layout_impl(args, max_blocks, 0);  // the two-dimensional grid has no sets
  return (int)(groups * 8);
}
int tick_args_layout(TickArgs &args, int max_blocks, int share) { return tick_args_layout_impl(args, max_blocks, share); }
int tick_args_layout(TickArgsSmall &args, int max_blocks) { return tick_args_layout_impl(args, max_blocks, 0); }

void tick_items_order(const TickItem *items, int n, bool sort, int share, int *order) {
  for (int i = 0; i < n; ++i) order[i] = i;
  if (!sort) return;
  std::stable_sort(order, order + n, [&](int a, int b) {
    const TickItem &x = items[a], &y = items[b];
    const int kx = x.res_blocks ? item_res_steps(x) : 0, ky = y.res_blocks ? item_res_steps(y) : 0;
    if (kx != ky || share <= 0) return kx > ky;
    // one reference level's items together (a RefLevelDesc is one level of one keyframe), by current level inside the run
    if (x.ref != y.ref) return std::less<const void *>()(x.ref, y.ref);
    return std::less<const void *>()(x.cur, y.cur);
  });
}

int tick_args_locate(const TickArgs &args, unsigned block, int *bx) {
  *bx = -1;
  if (!args.compact || (block >> 3) >= (unsigned)args.group_first[args.n_items]) return -1;
  int idx = -1;
  for (int i = 0; i <= args.n_items; ++i)
    if ((unsigned)args.group_first[i] <= (block >> 3)) idx = i;
  if (idx < 0 || idx >= args.n_items) return -1;
  int b;
  idx = tick_place(args, idx, (int)(block >> 3) - (int)args.group_first[idx], block, b);
  if (idx >= args.n_items || b >= (int)args.items[idx].res_blocks + (int)args.items[idx].ll_blocks) return -1;  // a surplus block: exits at once
  *bx = b;
  return idx;
}

hipError_t launch_tick_small(const TickArgsSmall &args, int max_blocks, hipStream_t stream, hipEvent_t t_start, hipEvent_t t_stop) {
  if (acc_mode() != 1) return hipErrorNotSupported;  // (with or without the reciprocal table: launch_tick decides)
  if (args.n_items <= 0 || max_blocks <= 0) return hipSuccess;
  LaunchGuard guard;
  dim3 grid((unsigned)((max_blocks + 7) & ~7), (unsigned)args.n_items, 1);
  if (args.compact) grid = dim3((unsigned)args.group_first[args.n_items] * 8u, 1, 1);
  if (t_start && t_stop) {
    void *kargs[] = {const_cast<TickArgsSmall *>(&args)};
    const void *kernel = args.rcp.nibbles ? reinterpret_cast<const void *>(&k_tick_small<2>)
                         : args.rcp.table ? reinterpret_cast<const void *>(&k_tick_small<1>)
                                          : reinterpret_cast<const void *>(&k_tick_small<0>);
    const hipError_t e = hipExtLaunchKernel(kernel, grid, dim3(kBlockThreads), kargs, 0, stream, t_start, t_stop, 0);
    if (e != hipSuccess) return e;
  } else if (args.rcp.nibbles) {
    hipLaunchKernelGGL(k_tick_small<2>, grid, dim3(kBlockThreads), 0, stream, args);
  } else if (args.rcp.table) {
    hipLaunchKernelGGL(k_tick_small<1>, grid, dim3(kBlockThreads), 0, stream, args);
  } else {
    hipLaunchKernelGGL(k_tick_small<0>, grid, dim3(kBlockThreads), 0, stream, args);
  }
  return hipGetLastError();
}

hipError_t launch_tick(const TickArgs &args, int max_blocks, hipStream_t stream, hipEvent_t t_start, hipEvent_t t_stop) {
  // the host-rcpps mode is built for the default accumulator only: under DVO_AMD_ACCUM=valu (the cross-check of the summation) it
  // is refused rather than silently run on the matrix pipe (dvo_amd_set_reciprocal_mode refuses first, with the reason)
  if (args.rcp.table && acc_mode() == 0) return hipErrorNotSupported;
  TickKernel kernel = pick_tick_kernel(args.rcp);
  if (args.n_items <= 0 || max_blocks <= 0) return hipSuccess;
  LaunchGuard guard;
  dim3 grid((unsigned)((max_blocks + 7) & ~7), (unsigned)args.n_items, 1);
  if (args.compact) grid = dim3((unsigned)args.group_first[args.n_items] * 8u, 1, 1);
  if (t_start && t_stop) {
    void *kargs[] = {const_cast<TickArgs *>(&args)};
    const hipError_t e = hipExtLaunchKernel(reinterpret_cast<const void *>(kernel), grid, dim3(kBlockThreads), kargs, 0, stream,
                                            t_start, t_stop, 0);
    if (e != hipSuccess) return e;
  } else {
    hipLaunchKernelGGL(kernel, grid, dim3(kBlockThreads), 0, stream, args);
  }
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// finalize: one 512-thread block per job.  Sums the 87 moments over the blocks in fp64, combines the ordered part of the
// records (count, S under both start parities, boundary residual/weight) left to right, locates the log-likelihood
// cut, sums the log-likelihood partials.
// ------------------------------------------------------------------------------------------------------------------
#ifndef DVO_FIN_THREADS
#define DVO_FIN_THREADS 512  // measured 384 / 448 / 512 / 640 / 1024: 512 schedules best next to other streams' k_tick blocks
#endif
constexpr int kFinThreads = DVO_FIN_THREADS;
constexpr int kFinSegThreads = 64;    // wave 0: the ordered part of the records (no block barriers inside)
constexpr int kFinAccFirst = 64;      // threads [64, ...): row-chunks x 24 groups of 4 columns (waves 1.. sum the moments)
constexpr int kFinCols = 96;
static_assert(kLevelChunksMax == 16, "finalize_block spells the tree over the 16 moment slices out");
constexpr int kFinCol4 = kFinCols / 4;
constexpr int kFinThreadsBatch = 256;  // the launch of a tick of many pairs: half the block runs 2 % more pairs/s next to other
                                       // streams' k_tick blocks (a small tick keeps 512 threads: its level-0 reduce is bandwidth)
// The reducer follows the level's summation tree (dvo_types.h, kLevelChunks): per chunk a fold in ascending block order, then a
// perfect binary tree over the 16 slices -- the same additions in the same order whether the 512-thread form (a single match())
// or the 256-thread form (a tick of many pairs) runs, and whether the item is a whole level or a band of it.  The 512-thread
// form gives every slice its own threads; in the 256-thread form a thread owns slices 2k and 2k + 1 and adds the two itself
// (the first level of the tree).
template <int NT>
struct FinGeometry {
  static constexpr int kChunks = NT == kFinThreadsBatch ? kLevelChunksMax / 2 : kLevelChunksMax;  // leaf slices the block's threads cover
  static constexpr int kPerThread = kLevelChunksMax / kChunks;                                 // slices per thread
  static_assert(kFinAccFirst + kChunks * kFinCol4 <= NT && kFinAccFirst + kNumAcc + 1 <= NT, "the block holds the summing and the output threads");
};

struct SegRec {
  int c;
  float first_w, l0, l1;
  double s0[3], s1[3];
};

// record of (a followed by b)
__device__ __forceinline__ SegRec seg_combine(const SegRec &a, const SegRec &b) {
  if (b.c == 0) return a;
  if (a.c == 0) return b;
  SegRec o;
  const bool flip = (a.c & 1) != 0;
  const double rxx = (double)a.l0 * a.l0, rxy = (double)a.l0 * a.l1, ryy = (double)a.l1 * a.l1;
  for (int i = 0; i < 3; ++i) {
    o.s0[i] = a.s0[i] + (flip ? b.s1[i] : b.s0[i]);
    o.s1[i] = a.s1[i] + (flip ? b.s0[i] : b.s1[i]);
  }
  // b starts on an odd rank under exactly one of the two hypotheses: there its first pixel pairs with a's last
  double *tgt = flip ? o.s0 : o.s1;
  tgt[0] += (double)b.first_w * rxx, tgt[1] += (double)b.first_w * rxy, tgt[2] += (double)b.first_w * ryy;
  o.c = a.c + b.c;
  o.first_w = a.first_w;
  o.l0 = b.l0, o.l1 = b.l1;
  return o;
}

// Diagnostic only (DVO_AMD_FIN_STAMPS=1): shader-clock stamps of the phases of block 0, read back by
// dvo_amd_debug_finalize_stamps().  Never read by any kernel; no output depends on them.
__device__ unsigned long long g_fin_stamps[8];
#define DVO_FIN_STAMP(i)                                                                  \
  do {                                                                                    \
    if (stamps && threadIdx.x == 0) g_fin_stamps[i] = __builtin_amdgcn_s_memtime(); \
  } while (0)


typedef unsigned v4u __attribute__((ext_vector_type(4)));
// one lane, one instruction, 16 bytes, system scope: the unit every record travels in (FinWire)
// (s_nop: a store of more than 8 bytes reads its data registers over several cycles, and the compiler's hazard recogniser
// does not see through inline assembly -- without it the next vector instruction may overwrite the tail of the data)
__device__ __forceinline__ void st16_system(DVO_GLOBAL void *p, v4u v) {
  asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
}
__device__ __forceinline__ v4u ld16_system(const DVO_GLOBAL void *p) {
  v4u v;
  asm volatile("global_load_dwordx4 %0, %1, off sc0 sc1\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
  return v;
}
// piece i of a record: two 8-byte halves {payload word, tag} (FinWire)
__device__ __forceinline__ v4u wire_piece(const unsigned *record_words, int i, unsigned tag) {
  v4u piece;
  piece.x = record_words[2 * i];
  piece.y = tag;
  piece.z = 2 * i + 1 < kFinWords ? record_words[2 * i + 1] : 0u;
  piece.w = tag;
  return piece;
}

// The one-hop exchange of a tile-sharded pair, run by the waves of k_finalize once the rank's record stands in LDS: wave
// (p mod n_waves) pushes it into rank p's exchange buffer as tagged 16-byte pieces, then every lane waits -- bounded -- for
// "its" pieces of rank p's record of this tick to land in the local buffer and forwards them, tag included, to the host.
// No fence and no ready word anywhere: a piece is valid when its tag is the tick.  Returns false on a timeout.
// The exchange description stays in memory and is read through the constant address space (scalar loads, the peer table
// indexed dynamically): a by-value copy with a dynamically indexed array would live in scratch.
__device__ bool exchange_records(const ExchangeArgs *xa, const unsigned *own_record, unsigned seq, int wave, int n_waves, int lane) {
  const DVO_CONST ExchangeArgs *a = (const DVO_CONST ExchangeArgs *)xa;
  const int n_ranks = a->n_ranks, rank = a->rank;
  const unsigned long long timeout = (unsigned long long)a->timeout_ticks;
  const int slot = (int)(seq & 1u) * n_ranks;
  bool ok = true;
  for (int p = wave; p < n_ranks; p += n_waves) {
    FinWire *dst = a->peers[p] + slot + rank;
    for (int i = lane; i < kFinWirePieces; i += kWave) st16_system((DVO_GLOBAL void *)dst->piece[i], wire_piece(own_record, i, seq));
  }
  const FinWire *local = a->local;
  FinWire *host_records = a->host_records;
  for (int p = wave; p < n_ranks; p += n_waves) {
    const FinWire *in = local + slot + p;
    FinWire *out = host_records + p;
    for (int i = lane; i < kFinWirePieces; i += kWave) {
      const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
      v4u piece = ld16_system((const DVO_GLOBAL void *)in->piece[i]);
      while (piece.y != seq || piece.w != seq) {  // both halves of the piece carry the tick (FinWire)
        __builtin_amdgcn_s_sleep(8);
        if (__builtin_amdgcn_s_memrealtime() - t0 > timeout) {
          ok = false;
          break;
        }
        piece = ld16_system((const DVO_GLOBAL void *)in->piece[i]);
      }
      if (piece.y == seq && piece.w == seq) st16_system((DVO_GLOBAL void *)out->piece[i], piece);
    }
  }
  return ok;
}

// One block per job.  Wave 0 folds the ordered part of the block records (count, S under both start parities, boundary
// residual / weight) left to right and locates the log-likelihood cut; waves 1.. sum the 87 moments and the
// log-likelihood partials in fp64 with 16-byte loads, eight in flight per thread.  Two block barriers in all; the record is
// assembled in LDS and pushed to the pinned host buffer as self-validating 16-byte pieces (FinWire): no fence, no ready word.
// One block reduces one item (see above); `exchange`: the tile-sharded pair's one-hop exchange instead of the hand-off to the host.
// EXCHANGE is a compile-time property of the launch: the batch and single-pair kernels carry no trace of the exchange tail.
template <int NT, bool EXCHANGE>
__device__ __forceinline__ void finalize_block(const FinItem &it, const bool stamps, const ExchangeArgs *exchange, const unsigned xseq) {
  constexpr int kFinChunks = FinGeometry<NT>::kChunks;
  const int t = threadIdx.x;
  __shared__ double sh_acc[kFinChunks][kFinCols];
  __shared__ SegRec sh_seg[kFinSegThreads];
  __shared__ int sh_cnt[kFinSegThreads];
  __shared__ __attribute__((aligned(16))) FinOut sh_out;

  DVO_FIN_STAMP(0);
  const gcf recs = (gcf)it.records;  // indexed by logical block of the level
  const int nb = it.records ? (int)it.n_blocks : 0;
  const int band_lo = (int)it.block_first, band_hi = band_lo + nb;  // the blocks this item reduces
  const int level_nb = (int)it.level_blocks;                        // the blocks the level's chunks partition
  const DVO_GLOBAL Q7Rec *const q7 =
      it.q7_off256 ? (const DVO_GLOBAL Q7Rec *)((const DVO_GLOBAL char *)it.ll_partials + 256u * (unsigned)it.q7_off256) : nullptr;
  if (t < kFinSegThreads) {
    // Wave 0: the ordered part.  Lane 4 c + q owns quarter q of chunk c (what of it lies in the band), folds its records in
    // ascending order, and the 64 lane records are folded by a binary tree -- chunk subtrees first, then the tree over chunks.
    SegRec r;
    r.c = 0, r.first_w = 0.0f, r.l0 = r.l1 = 0.0f;
    for (int i = 0; i < 3; ++i) r.s0[i] = r.s1[i] = 0.0;
    int b_lo, b_end;
    leaf_range(level_nb, 6, t, &b_lo, &b_end);
    b_lo = b_lo > band_lo ? b_lo : band_lo, b_end = b_end < band_hi ? b_end : band_hi;
    if (b_end < b_lo) b_end = b_lo;
    // four records' headers (64 bytes each) in flight at a time; the per-wave counts of the first four are kept in registers
    // for the prefix pass below, so a lane with at most four records (every level up to 256 blocks) reads its headers once
    // (the 256-thread batch form keeps two in flight: it is built for 96 registers, see k_finalize)
    constexpr int kHdr = NT == kFinThreadsBatch ? 2 : 4;
    unsigned cw_first[4][4] = {};
    for (int b0 = b_lo; b0 < b_end; b0 += kHdr) {
      v4f h0[kHdr], h1[kHdr], h2[kHdr], h3[kHdr];
#pragma unroll
      for (int k = 0; k < kHdr; ++k)
        if (b0 + k < b_end) {
          const gcf4 hp = reinterpret_cast<gcf4>(recs + (size_t)(b0 + k) * kRecStride);
          h0[k] = hp[0], h1[k] = hp[1], h2[k] = hp[2], h3[k] = hp[3];
        }
#pragma unroll
      for (int k = 0; k < kHdr; ++k)
        if (b0 + k < b_end) {
          SegRec q;
          q.c = (int)f2u(h0[k].x);
          q.first_w = h0[k].y, q.l0 = h0[k].z, q.l1 = h0[k].w;
          q.s0[0] = h1[k].x, q.s0[1] = h1[k].y, q.s0[2] = h1[k].z;
          q.s1[0] = h1[k].w, q.s1[1] = h2[k].x, q.s1[2] = h2[k].y;
          r = seg_combine(r, q);
          const int j = b0 - b_lo + k;  // the lane's j-th record
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            if (j == jj) cw_first[jj][0] = f2u(h2[k].z), cw_first[jj][1] = f2u(h2[k].w), cw_first[jj][2] = f2u(h3[k].x), cw_first[jj][3] = f2u(h3[k].y);
        }
    }
    const int own_total = r.c;
    sh_seg[t] = r;
    sh_cnt[t] = r.c;
    DVO_WAVE_LDS_SYNC();
    // ordered combine (binary tree over the 64 lanes; an empty record is the identity of seg_combine, bit for bit) and inclusive
    // scan of the per-lane valid counts: wave-local steps
    for (int stride = 1; stride < kFinSegThreads; stride <<= 1) {
      SegRec merged;
      int add = 0;
      const bool do_merge = (t % (2 * stride)) == 0;
      if (do_merge) merged = seg_combine(sh_seg[t], sh_seg[t + stride]);
      if (t >= stride) add = sh_cnt[t - stride];
      DVO_WAVE_LDS_SYNC();
      if (do_merge) sh_seg[t] = merged;
      sh_cnt[t] += add;
      DVO_WAVE_LDS_SYNC();
    }
    if (nb > 0) {
      if (t == 0) {
        const SegRec &a = sh_seg[0];
        sh_out.valid = a.c;
        sh_out.has_res = 1;
        // (host-rcpps mode, whole levels only: what the exact weights of the pass's last V mod 4 pixels add -- k_q7_tail)
        for (int i = 0; i < 3; ++i) sh_out.S[i] = a.s0[i] + (q7 ? q7->S[i] : 0.0), sh_out.S_odd[i] = a.s1[i];
        sh_out.first_w = a.first_w, sh_out.last_r0 = a.l0, sh_out.last_r1 = a.l1;
      }
      // exclusive scan of the valid counts over the band's wave segments: the log-likelihood pass needs each pixel's
      // rank to honour the V % 50 cut (Q6)
      int prefix = sh_cnt[t] - own_total;  // valid pixels of the band before this lane's blocks
      DVO_GLOBAL int *sp = (DVO_GLOBAL int *)it.seg_prefix_out;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (b_lo + k < b_end) {
#pragma unroll
          for (int wv = 0; wv < 4; ++wv) {
            sp[(b_lo + k) * kWavesPerBlock + wv] = prefix;
            prefix += (int)cw_first[k][wv];
          }
        }
      for (int b0 = b_lo + 4; b0 < b_end; b0 += 4) {  // levels with more than 256 blocks: the rest is read again
        v4f h2[4], h3[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (b0 + k < b_end) {
            const gcf4 hp = reinterpret_cast<gcf4>(recs + (size_t)(b0 + k) * kRecStride);
            h2[k] = hp[2], h3[k] = hp[3];
          }
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (b0 + k < b_end) {
            const int cw[4] = {(int)f2u(h2[k].z), (int)f2u(h2[k].w), (int)f2u(h3[k].x), (int)f2u(h3[k].y)};
            for (int wv = 0; wv < 4; ++wv) {
              sp[(b0 + k) * kWavesPerBlock + wv] = prefix;
              prefix += cw[wv];
            }
          }
      }
    } else if (t == 0) {
      sh_out.valid = 0;
      sh_out.has_res = 0;
      for (int i = 0; i < 3; ++i) sh_out.S[i] = 0.0, sh_out.S_odd[i] = 0.0;
      sh_out.first_w = sh_out.last_r0 = sh_out.last_r1 = 0.0f;
    }
  } else if (t >= kFinAccFirst && (t - kFinAccFirst) / kFinCol4 < kFinChunks) {
    // moments: 16-byte loads (4 columns).  A chunk's rows are added up in ascending order (the loads of several rows are in
    // flight at a time, the additions stay sequential)
    constexpr int kPer = FinGeometry<NT>::kPerThread;
    constexpr int kInFlight = 4;
    const int c4 = (t - kFinAccFirst) % kFinCol4, tc = (t - kFinAccFirst) / kFinCol4;
    double s[kPer][4];
#pragma unroll
    for (int v = 0; v < kPer; ++v) {
      s[v][0] = s[v][1] = s[v][2] = s[v][3] = 0.0;
      const int c = tc * kPer + v;  // the slice
      if (c4 * 4 < kNumAcc) {
        int lo, hi;
        leaf_range(level_nb, 4, c, &lo, &hi);
        lo = lo > band_lo ? lo : band_lo, hi = hi < band_hi ? hi : band_hi;
        const gcf base = recs + kRecAcc + c4 * 4;
        int b = lo;
        for (; b + kInFlight <= hi; b += kInFlight) {
          v4f r[kInFlight];
#pragma unroll
          for (int k = 0; k < kInFlight; ++k) r[k] = *reinterpret_cast<gcf4>(base + (size_t)(b + k) * kRecStride);
#pragma unroll
          for (int k = 0; k < kInFlight; ++k)
            s[v][0] += (double)r[k].x, s[v][1] += (double)r[k].y, s[v][2] += (double)r[k].z, s[v][3] += (double)r[k].w;
        }
        for (; b < hi; ++b) {
          const v4f r0 = *reinterpret_cast<gcf4>(base + (size_t)b * kRecStride);
          s[v][0] += (double)r0.x, s[v][1] += (double)r0.y, s[v][2] += (double)r0.z, s[v][3] += (double)r0.w;
        }
      } else if (c4 == (kNumAcc + 3) / 4) {
        // the first spare column group sums the log-likelihood partials: the first slice of a chunk folds the chunk's merged
        // blocks in ascending order, the chunk's other slices add exact zeros
        const int m_log2 = (int)it.ll_merge_log2, ll_nb = (int)it.ll_level_blocks;
        const int per = 4 - level_chunks_log2(ll_nb);
        int lo = 0, hi = 0;
        if ((c & ((1 << per) - 1)) == 0) lo = ll_blocks_before(ll_nb, m_log2, c >> per), hi = ll_blocks_before(ll_nb, m_log2, (c >> per) + 1);
        const int ll_lo = (int)it.ll_first, ll_hi = ll_lo + (int)it.n_ll_blocks;
        lo = lo > ll_lo ? lo : ll_lo, hi = hi < ll_hi ? hi : ll_hi;
        const DVO_GLOBAL double *llp = (const DVO_GLOBAL double *)it.ll_partials;
        const DVO_GLOBAL float *qp = (const DVO_GLOBAL float *)((const DVO_GLOBAL double *)it.ll_partials + it.ll_qmax_off);
        float qm = 0.0f;
        for (int b = lo; b < hi; ++b) s[v][0] += llp[b], qm = __builtin_fmaxf(qm, qp[b]);
        s[v][1] = (double)qm;  // (rides in the second column of the spare group)
      }
    }
    if (kPer == 2) {  // chunks 2k and 2k + 1 meet here: the first level of the tree (the 512-thread form adds them after the barrier)
      const bool is_ll = c4 * 4 >= kNumAcc;
      s[0][0] += s[kPer - 1][0], s[0][2] += s[kPer - 1][2], s[0][3] += s[kPer - 1][3];
      s[0][1] = is_ll ? (s[kPer - 1][1] > s[0][1] ? s[kPer - 1][1] : s[0][1]) : s[0][1] + s[kPer - 1][1];
    }
    sh_acc[tc][c4 * 4 + 0] = s[0][0], sh_acc[tc][c4 * 4 + 1] = s[0][1];
    sh_acc[tc][c4 * 4 + 2] = s[0][2], sh_acc[tc][c4 * 4 + 3] = s[0][3];
  }
  __syncthreads();
  DVO_FIN_STAMP(1);

  // chunk sums -> totals: the perfect binary tree over the 16 slices
  constexpr bool kPaired = FinGeometry<NT>::kPerThread == 2;  // the threads added chunks 2k and 2k + 1 already
  auto tree = [&](const int col) __attribute__((always_inline)) {
    double p[kLevelChunksMax / 2];
#pragma unroll
    for (int k = 0; k < kLevelChunksMax / 2; ++k) p[k] = kPaired ? sh_acc[k][col] : sh_acc[kPaired ? k : 2 * k][col] + sh_acc[kPaired ? k : 2 * k + 1][col];
    return ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));
  };
  if (t >= kFinAccFirst && t < kFinAccFirst + kNumAcc)
    sh_out.acc[t - kFinAccFirst] = tree(t - kFinAccFirst) + (q7 ? q7->acc[t - kFinAccFirst] : 0.0);
  if (t == kFinAccFirst + kNumAcc) {
    double qm = 0.0;
    for (int c = 0; c < kFinChunks; ++c) qm = sh_acc[c][89] > qm ? sh_acc[c][89] : qm;
    sh_out.ll_sum = tree(88);
    sh_out.ll_qmax = (float)qm;
    sh_out.has_ll = it.n_ll_blocks > 0 ? 1 : 0;
  }
  __syncthreads();
  DVO_FIN_STAMP(2);

  // ---- tile-sharded pair: the record goes to the peers instead, theirs come back to the host (see exchange_records)
  if (EXCHANGE && exchange && blockIdx.x == 0) {
    __shared__ int sh_bad;
    if (t == 0) sh_bad = 0;
    __syncthreads();
    if (!exchange_records(exchange, reinterpret_cast<const unsigned *>(&sh_out), xseq, t >> 6, NT / kWave, t & (kWave - 1)))
      atomicOr(&sh_bad, 1);
    __syncthreads();
    if (t == 0 && sh_bad)
      __hip_atomic_store(((const DVO_CONST ExchangeArgs *)exchange)->host_seq, xseq | 0x80000000u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  // ---- publish: every piece of the record goes to the pinned host buffer with the tick's sequence number inside it, in one
  // 16-byte system-scope store per lane.  The host validates piece by piece (FinWire), so nothing is fenced or ordered here.
  static_assert(kFinWirePieces <= 256, "one lane per piece in the smallest finalize block");
  if (t < kFinWirePieces)
    st16_system((DVO_GLOBAL void *)it.out->piece[t], wire_piece(reinterpret_cast<const unsigned *>(&sh_out), t, it.seq));
  if (it.out_dev && t < (int)(sizeof(FinOut) / 16))  // device copy for the collective fallback of a tile-sharded pair
    ((DVO_GLOBAL v4f *)it.out_dev)[t] = reinterpret_cast<const v4f *>(&sh_out)[t];
  DVO_FIN_STAMP(3);
}

// The batch form (256 threads) is built for under 96 registers and 11 KB of LDS (beside 4 x 36.5 KB of k_tick blocks).  Until the
// Gram matrix moved to nine tiles a SIMD full of k_tick waves (4 x 104 registers) had 96 left and a reducer block could start on
// a full CU; with 4 x 128 it takes the place of the next k_tick block that retires there (one retires somewhere every ~20 ns).
template <int NT, bool EXCHANGE>
__global__ __launch_bounds__(NT, NT == kFinThreadsBatch ? 5 : 1) void k_finalize(const FinArgs args) {
  // A reducer block is a few thousand cycles of work on the critical path of its group's tick, started on a CU whose SIMDs are
  // busy with four k_tick waves each: at the default priority it gets a fifth of the issue slots and takes twice as long as alone
  // on the GPU.  (DVO_AMD_FIN_PRIORITY=0 turns this off for an A/B.)
  if (args.pad2 & kFinFlagPriority) __builtin_amdgcn_s_setprio(3);
  finalize_block<NT, EXCHANGE>(args.items[blockIdx.x], args.pad == 0x57A3 && blockIdx.x == 0,
                               EXCHANGE && blockIdx.x == 0 ? args.exchange : nullptr, args.xseq);
}

// the same behind the small argument block of a tick of at most kMaxSmallItems pairs
__global__ __launch_bounds__(kFinThreads) void k_finalize_small(const FinArgsSmall args) {
  finalize_block<kFinThreads, false>(args.items[blockIdx.x], args.pad == 0x57A3 && blockIdx.x == 0, nullptr, 0u);
}

// The one-hop exchange of a ready-made record (device memory): the rare second exchange of a tick of a tile-sharded pair -- the
// band-edge terms of the reference's 50-term likelihood products (dvo_sharded.cpp: sharded_overflow) travel as a FinOut-shaped
// record through the same mapped buffers, tags and generations as the tick records do.
__global__ __launch_bounds__(kFinThreadsBatch) void k_exchange_record(const FinOut *__restrict__ rec, const ExchangeArgs *exchange, unsigned xseq) {
  __shared__ __attribute__((aligned(16))) FinOut sh_out;
  __shared__ int sh_bad;
  const int t = threadIdx.x;
  if (t < (int)(sizeof(FinOut) / 16)) reinterpret_cast<v4f *>(&sh_out)[t] = reinterpret_cast<const v4f *>(rec)[t];
  if (t == 0) sh_bad = 0;
  __syncthreads();
  if (!exchange_records(exchange, reinterpret_cast<const unsigned *>(&sh_out), xseq, t >> 6, kFinThreadsBatch / kWave, t & (kWave - 1)))
    atomicOr(&sh_bad, 1);
  __syncthreads();
  if (t == 0 && sh_bad)
    __hip_atomic_store(((const DVO_CONST ExchangeArgs *)exchange)->host_seq, xseq | 0x80000000u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

hipError_t launch_exchange_record(const FinOut *rec_dev, const ExchangeArgs *exchange_dev, unsigned xseq, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_exchange_record, dim3(1), dim3(kFinThreadsBatch), 0, stream, rec_dev, exchange_dev, xseq);
  return hipGetLastError();
}

// A dispatch whose only purpose is its name in a profiler's dispatch table: bench.py brackets its single-stream timing pass with
// two of them, and the summaries of the counter passes (dvo_slam_amd/pmc.py) select exactly the k_tick dispatches in between.
__global__ void k_marker(unsigned *sink, unsigned tag) {
  if (sink && tag == 0xFFFFFFFFu) *sink = tag;  // (never true: the kernel has no effect)
}
hipError_t launch_marker(unsigned tag, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_marker, dim3(1), dim3(64), 0, stream, (unsigned *)nullptr, tag & 0x7FFFFFFFu);
  return hipGetLastError();
}

// Which hardware queue does the runtime run this stream on?  One thread reports HW_ID's PIPE_ID (bits 7:6) and QUEUE_ID (bits
// 26:24) of the wave it runs in (context creation: host::pick_balanced_stream).
__global__ void k_queue_probe(unsigned *out) {
  unsigned hw;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  if (threadIdx.x == 0) __hip_atomic_store(out, 0x80000000u | (((hw >> 6) & 3u) << 3) | ((hw >> 24) & 7u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
hipError_t launch_queue_probe(unsigned *out_pinned, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_queue_probe, dim3(1), dim3(64), 0, stream, out_pinned);
  return hipGetLastError();
}

hipError_t launch_rcp_midpoint_probe(int k, unsigned *out_rn, unsigned *out_rtz, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_rcp_midpoint_probe, dim3((unsigned)(((1 << k) + 255) / 256)), dim3(256), 0, stream, k, out_rn, out_rtz);
  return hipGetLastError();
}

hipError_t launch_rcp_table_probe(const RcpTable &rcp, const float *in, float *out, int n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  LaunchGuard guard;
  hipLaunchKernelGGL(k_rcp_table_probe, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, rcp, in, out, n);
  return hipGetLastError();
}

// (trace builds only) copies up to `capacity` block records (5 x 64-bit words each: t0, t_first, t_end, info | hw << 32, 0) out and
// resets the trace; returns the number of blocks recorded, or -1 in a build without the trace
long long read_block_trace(unsigned long long *out, long long capacity) {
#ifdef DVO_TRACE_BLOCKS
  unsigned n = 0;
  if (hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_trace_n), sizeof(n)) != hipSuccess) return -2;
  const unsigned have = n < kTraceCapacity ? n : kTraceCapacity;
  const unsigned take = (long long)have < capacity ? have : (unsigned)capacity;
  if (out && take) {
    std::vector<BlockTrace> tmp(take);
    if (hipMemcpyFromSymbol(tmp.data(), HIP_SYMBOL(g_trace), sizeof(BlockTrace) * take) != hipSuccess) return -2;
    for (unsigned i = 0; i < take; ++i) {
      out[4 * i] = tmp[i].t0, out[4 * i + 1] = tmp[i].t_first, out[4 * i + 2] = tmp[i].t_end;
      out[4 * i + 3] = (unsigned long long)tmp[i].info | ((unsigned long long)tmp[i].hw << 32);
    }
  }
  const unsigned zero = 0;
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_trace_n), &zero, sizeof(zero));
  return (long long)n;
#else
  (void)out, (void)capacity;
  return -1;
#endif
}

hipError_t read_finalize_stamps(unsigned long long out[8]) {
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fin_stamps), sizeof(unsigned long long) * 8);
}

hipError_t launch_q7_tail(const Q7Args &args, hipStream_t stream) {
  if (args.n_items <= 0) return hipSuccess;
  LaunchGuard guard;
  hipLaunchKernelGGL(k_q7_tail, dim3((unsigned)args.n_items), dim3(kWave), 0, stream, args);
  return hipGetLastError();
}
hipError_t launch_q7_tail_small(const Q7ArgsSmall &args, hipStream_t stream) {
  if (args.n_items <= 0) return hipSuccess;
  LaunchGuard guard;
  hipLaunchKernelGGL(k_q7_tail_small, dim3((unsigned)args.n_items), dim3(kWave), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_finalize_small(const FinArgsSmall &args, hipStream_t stream) {
  if (args.n_items <= 0) return hipSuccess;
  LaunchGuard guard;
  hipLaunchKernelGGL(k_finalize_small, dim3((unsigned)args.n_items), dim3(kFinThreads), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_finalize(const FinArgs &args, hipStream_t stream) {
  if (args.n_items <= 0) return hipSuccess;
  LaunchGuard guard;
  if (args.exchange)
    hipLaunchKernelGGL((k_finalize<kFinThreads, true>), dim3((unsigned)args.n_items), dim3(kFinThreads), 0, stream, args);
  else if (args.n_items > kMaxSmallItems)
    hipLaunchKernelGGL((k_finalize<kFinThreadsBatch, false>), dim3((unsigned)args.n_items), dim3(kFinThreadsBatch), 0, stream, args);
  else
    hipLaunchKernelGGL((k_finalize<kFinThreads, false>), dim3((unsigned)args.n_items), dim3(kFinThreads), 0, stream, args);
  return hipGetLastError();
}

hipError_t launch_ll_overflow(const float2 *res, const int *seg_prefix, int seg_first, int n_segs, int seg_px, int rank_offset,
                              int n_px, int cut_rank, int rank_end, const float P[4], unsigned *result_host, hipStream_t stream) {
  if (n_segs <= 0) return hipSuccess;
  LaunchGuard guard;
  const int segs_per_block = 8;
  hipLaunchKernelGGL(k_ll_overflow, dim3((unsigned)((n_segs + segs_per_block - 1) / segs_per_block)), dim3(kWave), 0, stream, res,
                     seg_prefix, seg_first, n_segs, segs_per_block, seg_px, rank_offset, n_px, cut_rank, rank_end, P[0], P[1], P[2], P[3],
                     result_host);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// pyramid construction (all round-to-nearest, no contraction: bit-identical to the CPU restatement)
// ------------------------------------------------------------------------------------------------------------------

// pyrDownMeanSmooth<float> for intensity and pyrDownSubsample<float> for depth, rgbd_image.cpp:38-55,127-139
__global__ void k_pyr_down(const float *__restrict__ ip, const float *__restrict__ zp, int wp, float *__restrict__ io,
                           float *__restrict__ zo, int w, int h) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x >= w || y >= h) return;
  const float *r0 = ip + (size_t)(2 * y) * wp + 2 * x;
  const float *r1 = r0 + wp;
  io[(size_t)y * w + x] = (((r0[0] + r0[1]) + r1[0]) + r1[1]) / 4.0f;
  zo[(size_t)y * w + x] = zp[(size_t)(2 * y) * wp + 2 * x];
}

hipError_t launch_pyr_down(const float *i_prev, const float *z_prev, int w_prev, float *i_out, float *z_out, int w, int h,
                           hipStream_t stream) {
  LaunchGuard guard;
  dim3 grid((unsigned)((w + 255) / 256), (unsigned)h);
  hipLaunchKernelGGL(k_pyr_down, grid, dim3(256), 0, stream, i_prev, z_prev, w_prev, i_out, z_out, w, h);
  return hipGetLastError();
}

// calculateDerivativeX/Y (rgbd_image.cpp:419-472, rgbd_image_sse.cpp:241-284), buildAccelerationStructure (:534-543) in
// the gather layout, the planar copies the reference side reads, and the pixel-ray tables of RgbdCamera (:186-204)
__global__ void k_level_planes(const float *__restrict__ ip, const float *__restrict__ zp, int w, int h, int n_pad, float fx,
                               float fy, float ox, float oy, float4 *__restrict__ c_a, float2 *__restrict__ c_b,
                               float *__restrict__ r_i, float *__restrict__ r_ix, float *__restrict__ r_iy,
                               float *__restrict__ tx, float *__restrict__ ty, int ty_len) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = w * h;
  if (i < w) tx[i] = ((float)i - ox) / fx;
  if (i < ty_len) ty[i] = ((float)i - oy) / fy;
  if (i >= n_pad) return;
  if (i >= n) {
    r_i[i] = 0.0f, r_ix[i] = 0.0f, r_iy[i] = 0.0f;
    return;
  }
  const int y = i / w, x = i - y * w;
  const int xp = x > 0 ? x - 1 : 0, xn = x < w - 1 ? x + 1 : w - 1;
  const int yp = y > 0 ? y - 1 : 0, yn = y < h - 1 ? y + 1 : h - 1;
  const float I = ip[i], Z = zp[i];
  const float Ix = (ip[y * w + xn] - ip[y * w + xp]) * 0.5f;
  const float Iy = (ip[yn * w + x] - ip[yp * w + x]) * 0.5f;
  const float Zx = (zp[y * w + xn] - zp[y * w + xp]) * 0.5f;
  const float Zy = (zp[yn * w + x] - zp[yp * w + x]) * 0.5f;
  c_a[i] = make_float4(I, Z, Ix, Iy);
  c_b[i] = make_float2(Zx, Zy);
  r_i[i] = I, r_ix[i] = Ix, r_iy[i] = Iy;
}

hipError_t launch_level_planes(const float *i_plane, const float *z_plane, int w, int h, int n_pad, float fx, float fy,
                               float ox, float oy, float4 *c_a, float2 *c_b, float *r_i, float *r_ix, float *r_iy,
                               float *tx, float *ty, int ty_len, hipStream_t stream) {
  LaunchGuard guard;
  int span = n_pad > ty_len ? n_pad : ty_len;
  if (w > span) span = w;
  hipLaunchKernelGGL(k_level_planes, dim3((unsigned)((span + 255) / 256)), dim3(256), 0, stream, i_plane, z_plane, w, h,
                     n_pad, fx, fy, ox, oy, c_a, c_b, r_i, r_ix, r_iy, tx, ty, ty_len);
  return hipGetLastError();
}

// ValidPointAndGradientThresholdPredicate::isPointOk (point_selection.h:63-66) applied in place: zsel = z where the pixel
// is selected, NaN elsewhere (and in the padding).  Count and last selected index (selectPointsFromImage's running output
// pointer, point_selection.cpp:119-152) leave every block as one {count, last index} pair -- no atomics: 10 000 same-address
// atomics of a 640x480 level serialise to 100 us, the kernel streams its 9 MB in a tenth of that.
__global__ __launch_bounds__(256) void k_select(const float *__restrict__ zp, const float4 *__restrict__ c_a,
                                                const float2 *__restrict__ c_b, int n, int n_pad, float ti, float td,
                                                float *__restrict__ zsel, int2 *__restrict__ block_partials) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float out = u2f(0x7fc00000u);
  bool ok = false;
  if (i < n) {
    const float z = zp[i];
    const float4 a = c_a[i];
    const float2 b = c_b[i];
    ok = (z == z) && (b.x == b.x) && (b.y == b.y) &&
         (__builtin_fabsf(a.z) > ti || __builtin_fabsf(a.w) > ti || __builtin_fabsf(b.x) > td || __builtin_fabsf(b.y) > td);
    if (ok) out = z;
  }
  if (i < n_pad) zsel[i] = out;
  __shared__ int sh_cnt[4], sh_last[4];
  const unsigned long long m = __ballot(ok);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh_cnt[wave] = __popcll(m);
    sh_last[wave] = m ? (int)(blockIdx.x * blockDim.x) + wave * kWave + (63 - __builtin_clzll(m)) : -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0, last = -1;
    for (int w = 0; w < 4; ++w) c += sh_cnt[w], last = sh_last[w] > last ? sh_last[w] : last;
    block_partials[blockIdx.x] = make_int2(c, last);
  }
}

// one block: the level's count and last selected index from the block partials, then Q3 -- computeResidualsSse walks the
// selection two points at a time and never looks at an odd trailing point (dense_tracking_impl.cpp:169-171)
__global__ __launch_bounds__(256) void k_select_finish(const int2 *__restrict__ block_partials, int n_blocks, float *zsel,
                                                       int *__restrict__ counters) {
  int c = 0, last = -1;
  for (int b = threadIdx.x; b < n_blocks; b += 256) {
    const int2 p = block_partials[b];
    c += p.x, last = p.y > last ? p.y : last;
  }
  __shared__ int sh_c[256], sh_l[256];
  sh_c[threadIdx.x] = c, sh_l[threadIdx.x] = last;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh_c[threadIdx.x] += sh_c[threadIdx.x + s];
      sh_l[threadIdx.x] = sh_l[threadIdx.x + s] > sh_l[threadIdx.x] ? sh_l[threadIdx.x + s] : sh_l[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counters[0] = sh_c[0], counters[1] = sh_l[0];
    if ((sh_c[0] & 1) && sh_l[0] >= 0) zsel[sh_l[0]] = u2f(0x7fc00000u);
  }
}

hipError_t launch_select(const float *z_plane, const float4 *c_a, const float2 *c_b, int n, int n_pad, float ti, float td,
                         float *zsel, int *counters, int2 *block_partials, hipStream_t stream) {
  LaunchGuard guard;
  const int n_blocks = (n_pad + 255) / 256;
  hipLaunchKernelGGL(k_select, dim3((unsigned)n_blocks), dim3(256), 0, stream, z_plane, c_a, c_b, n, n_pad, ti, td, zsel,
                     block_partials);
  hipLaunchKernelGGL(k_select_finish, dim3(1), dim3(256), 0, stream, (const int2 *)block_partials, n_blocks, zsel, counters);
  return hipGetLastError();
}

// k_select behind a selection mask (dvo_amd_mask, dvo_mask.cpp): keep = mask[i] != 0 && the threshold predicate.  The mask is a
// byte plane of the level in scan order, so a wave's 64 bytes are one coalesced load next to the 36 bytes per pixel k_select
// streams anyway.  Same zsel, same {count, last index} partials, one writer per pixel and no atomics: k_select_finish,
// k_select_prefix and k_compact run behind it unchanged, and the result cannot depend on the launch geometry.  A kernel of its
// own and not a template of k_select, so that the unmasked kernel stays the code it was.
__global__ __launch_bounds__(256) void k_select_masked(const float *__restrict__ zp, const float4 *__restrict__ c_a,
                                                       const float2 *__restrict__ c_b, const unsigned char *__restrict__ mask, int n,
                                                       int n_pad, float ti, float td, float *__restrict__ zsel,
                                                       int2 *__restrict__ block_partials) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float out = u2f(0x7fc00000u);
  bool ok = false;
  if (i < n) {
    const unsigned char keep = mask[i];
    const float z = zp[i];
    const float4 a = c_a[i];
    const float2 b = c_b[i];
    ok = keep != 0 && (z == z) && (b.x == b.x) && (b.y == b.y) &&
         (__builtin_fabsf(a.z) > ti || __builtin_fabsf(a.w) > ti || __builtin_fabsf(b.x) > td || __builtin_fabsf(b.y) > td);
    if (ok) out = z;
  }
  if (i < n_pad) zsel[i] = out;
  __shared__ int sh_cnt[4], sh_last[4];
  const unsigned long long m = __ballot(ok);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh_cnt[wave] = __popcll(m);
    sh_last[wave] = m ? (int)(blockIdx.x * blockDim.x) + wave * kWave + (63 - __builtin_clzll(m)) : -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0, last = -1;
    for (int w = 0; w < 4; ++w) c += sh_cnt[w], last = sh_last[w] > last ? sh_last[w] : last;
    block_partials[blockIdx.x] = make_int2(c, last);
  }
}

hipError_t launch_select_masked(const float *z_plane, const float4 *c_a, const float2 *c_b, const unsigned char *mask, int n, int n_pad,
                                float ti, float td, float *zsel, int *counters, int2 *block_partials, hipStream_t stream) {
  LaunchGuard guard;
  const int n_blocks = (n_pad + 255) / 256;
  hipLaunchKernelGGL(k_select_masked, dim3((unsigned)n_blocks), dim3(256), 0, stream, z_plane, c_a, c_b, mask, n, n_pad, ti, td, zsel,
                     block_partials);
  hipLaunchKernelGGL(k_select_finish, dim3(1), dim3(256), 0, stream, (const int2 *)block_partials, n_blocks, zsel, counters);
  return hipGetLastError();
}

// The planes of a selection mask (dvo_mask.cpp).  k_mask_plane: a level as the caller gave it (rows of `stride` bytes) into the
// mask's own packed plane, any non-zero byte as 1; src == dst with stride == w normalises a plane in place (every byte is read
// and written by the same lane).  k_mask_down: level l + 1 from the normalised level l, kept iff all (any_rule == 0) or any
// (any_rule != 0) of the four pixels under it are kept; an odd trailing row or column of the parent has no child, as in
// k_pyr_down.  Both count the kept pixels of the plane they write: one integer atomic per wave (ballots), as k_count_inside.
__global__ __launch_bounds__(256) void k_mask_plane(const unsigned char *src, int stride, unsigned char *dst, int w, int h,
                                                    int *__restrict__ kept) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  bool keep = false;  // (no early return: every lane takes part in the ballot)
  if (x < w && y < h) {
    keep = src[(size_t)y * stride + x] != 0;
    dst[(size_t)y * w + x] = keep ? 1 : 0;
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(kept, __popcll(m));
}

__global__ __launch_bounds__(256) void k_mask_down(const unsigned char *__restrict__ mp, int wp, unsigned char *__restrict__ mo, int w,
                                                   int h, int any_rule, int *__restrict__ kept) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  bool keep = false;
  if (x < w && y < h) {
    // 2 * x is even and the parent's rows are a multiple of 4 bytes long in a 256-byte aligned plane: two aligned 2-byte loads
    const unsigned char *r0 = mp + (size_t)(2 * y) * wp + 2 * x;
    const unsigned a = *(const unsigned short *)r0, b = *(const unsigned short *)(r0 + wp);
    keep = any_rule ? (a | b) != 0u : (a & b) == 0x0101u;
    mo[(size_t)y * w + x] = keep ? 1 : 0;
  }
  const unsigned long long m = __ballot(keep);
  if ((threadIdx.x & (kWave - 1)) == 0 && m) atomicAdd(kept, __popcll(m));
}

hipError_t launch_mask_plane(const unsigned char *src, int stride, unsigned char *dst, int w, int h, int *kept, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_mask_plane, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, stream, src, stride, dst, w, h, kept);
  return hipGetLastError();
}

hipError_t launch_mask_down(const unsigned char *m_prev, int w_prev, unsigned char *m_out, int w, int h, int any_rule, int *kept,
                            hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_mask_down, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, stream, m_prev, w_prev, m_out, w, h,
                     any_rule, kept);
  return hipGetLastError();
}

// ---- inlier masks from an alignment's residuals (dvo_amd_mask_from_residuals, dvo_mask_residual.cpp; the rule is pinned in
// include/dvo_amd.h under "Residual masks") ---------------------------------------------------------------------------------------
// k_residual_mask: ONE launch over all (pair, level) records of a call, laid out as k_mask_warp is: blockIdx.y walks the records,
// striding by gridDim.y, blockIdx.x a chunk of the reference level; a lane owns four consecutive pixels of one row.  It is a gather
// over the REFERENCE's pixels in the image, not over a compacted selection: four coalesced plane loads per lane (depth, {Zx, Zy},
// intensity), the residual stage of the tracker -- project_pixel_rtz<0> / gather_pixel / finish_pixel_rtz above, the very
// functions k_tick calls, in round-toward-zero behind k_tick's fencing -- then the Mahalanobis distance in round-to-nearest, every
// operation rounded on its own (this file is compiled without contraction), the verdict, one 32-bit store of four mask bytes and,
// when asked for, one 16-byte store of four distances.  Counts: ballots and popcounts per wave, LDS per block, one integer atomic
// per non-zero count, as k_mask_warp.
//
// Q3 (dense_tracking_impl.cpp:169-171): the tracker walks its point list two points at a time and never looks at an odd trailing
// point, so dvo_amd_residuals has no residual there.  Which pixel that is -- the last evaluated one of the level, if their number
// is odd -- is known only when the whole level has been counted: the blocks of a record count themselves done (kRmDone), and the
// block that draws the last number re-evaluates that one pixel and moves it to `invalid` in the plane, the distance plane and the
// counts.  The hand-off is the counter form of an agent-scope release / acquire: every wave waits for its own stores, the block
// meets at a barrier, one lane releases, waits and adds; the last arriver acquires.  Its patch is ordered behind every other
// block's stores by that chain, whatever XCD they ran on; the counts it reads were written by atomics and are read by atomics.

// the residual stage and the verdict for N pixels of one row (N = 4: a lane's pixels; N = 1: the Q3 pixel).  cls: -1 unevaluated,
// else kRmInvalid / kRmInlier / kRmOutlier; dist: the distance, NaN where there is none
template <int N>
__device__ __forceinline__ void residual_mask_pixels(const LevelPairDesc &d, const float *kt, const float *P, const float max_distance,
                                                     const float (&z_in)[N], const float (&zx)[N], const float (&zy)[N],
                                                     const float (&ri_in)[N], const float (&tx)[N], const float ty, int (&cls)[N],
                                                     float (&dist)[N]) {
  // ---- round-to-nearest: reference point = pixel ray * depth, as the residual pass forms it
  float x[N], y[N], z[N], ri[N];
#pragma unroll
  for (int k = 0; k < N; ++k) z[k] = z_in[k], ri[k] = ri_in[k], x[k] = tx[k] * z[k], y[k] = ty * z[k];
  // ---- switch to round-toward-zero: every float that crosses is made opaque on both sides of the s_setreg
#pragma unroll
  for (int k = 0; k < N; ++k) { DVO_OPAQUE(x[k]); DVO_OPAQUE(y[k]); DVO_OPAQUE(z[k]); DVO_OPAQUE(ri[k]); }
  round_toward_zero();
#pragma unroll
  for (int k = 0; k < N; ++k) { DVO_OPAQUE(x[k]); DVO_OPAQUE(y[k]); DVO_OPAQUE(z[k]); DVO_OPAQUE(ri[k]); }
  float r0[N], r1[N];
  bool ok[N];
  {
    Proj p[N];
    Gathered g[N];
#pragma unroll
    for (int k = 0; k < N; ++k) p[k] = project_pixel_rtz<0>(kt, d, x[k], y[k], z[k]);
#pragma unroll
    for (int k = 0; k < N; ++k) g[k] = gather_pixel(d, p[k].base);  // (a pixel that is not evaluated or falls outside gathers at 0)
#pragma unroll
    for (int k = 0; k < N; ++k) {
      float e2, e3, e4, e5;
      finish_pixel_rtz<true>(d, p[k], g[k], z[k], ri[k], 0.0f, 0.0f, r0[k], r1[k], e2, e3, e4, e5, ok[k]);
    }
  }
  // ---- back to round-to-nearest
#pragma unroll
  for (int k = 0; k < N; ++k) { DVO_OPAQUE(r0[k]); DVO_OPAQUE(r1[k]); }
  round_to_nearest();
#pragma unroll
  for (int k = 0; k < N; ++k) { DVO_OPAQUE(r0[k]); DVO_OPAQUE(r1[k]); }
#pragma unroll
  for (int k = 0; k < N; ++k) {
    // the validity predicate of the select kernels (k_select with thresholds of -1): z, Zx, Zy are no NaN
    const bool evaluated = (z_in[k] == z_in[k]) && (zx[k] == zx[k]) && (zy[k] == zy[k]);
    // mahalanobis() of computeWeightsSse, product by product, mean 0 (Q4): r^T P r with P column-major
    const float t0 = r0[k] * P[0] + r1[k] * P[1];
    const float t1 = r0[k] * P[2] + r1[k] * P[3];
    const float dd = t0 * r0[k] + t1 * r1[k];
    const bool valid = evaluated && ok[k];
    cls[k] = !evaluated ? -1 : !ok[k] ? (int)kRmInvalid : dd <= max_distance ? (int)kRmInlier : (int)kRmOutlier;  // (a NaN distance: outlier)
    dist[k] = valid ? dd : u2f(0x7fc00000u);
  }
}

// what a block needs of the current level's descriptor, through the constant address space as load_desc reads it
__device__ __forceinline__ LevelPairDesc residual_mask_desc(const CurLevelDesc *cur) {
  const DVO_CONST CurLevelDesc *c = (const DVO_CONST CurLevelDesc *)cur;
  LevelPairDesc d = {};
  d.c_a = c->c_a, d.c_b = c->c_b;
  d.w = c->w, d.h = c->h;
#pragma unroll
  for (int i = 0; i < 6; ++i) d.wc[i] = c->wc[i];
#pragma unroll
  for (int i = 0; i < 4; ++i) d.wr[i] = c->wr[i];
  d.ub_x = c->ub_x, d.ub_y = c->ub_y;
  return d;
}

__global__ void __launch_bounds__(kResidualMaskBlock) k_residual_mask(const ResidualMaskRecord *__restrict__ records, int n_records) {
  constexpr int kWaves = kResidualMaskBlock / kWave, kLanePixels = kResidualMaskLanePixels;
  constexpr int kCnt = 6;  // evaluated, invalid, inlier, outlier (the record's words), kept, index + 1 of the last evaluated pixel
  __shared__ unsigned s_cnt[kWaves][kCnt];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  for (int rec = blockIdx.y; rec < n_records; rec += gridDim.y) {
    const ResidualMaskRecord R = records[rec];  // uniform over the block
    if (blockIdx.x * kResidualMaskChunk >= R.n) continue;  // (block-uniform: no barrier is skipped by part of a block)
    const LevelPairDesc d = residual_mask_desc(R.cur);
    float kt[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) kt[i] = R.kt[i];
    const int p0 = (blockIdx.x * kResidualMaskBlock + threadIdx.x) * kLanePixels;
    const bool live = p0 < R.n;  // (n is a multiple of 4: four pixels or none, all in one row)
    const float qnan = u2f(0x7fc00000u);
    float z[kLanePixels] = {qnan, qnan, qnan, qnan}, zx[kLanePixels] = {qnan, qnan, qnan, qnan}, zy[kLanePixels] = {qnan, qnan, qnan, qnan};
    float ri[kLanePixels] = {0.f, 0.f, 0.f, 0.f}, tx[kLanePixels] = {0.f, 0.f, 0.f, 0.f};
    float ty = 0.f;
    if (live) {
      const float4 z4 = *(const float4 *)(R.z + p0), i4 = *(const float4 *)(R.ri + p0);
      const float4 za = *(const float4 *)(R.zd + p0), zb = *(const float4 *)(R.zd + p0 + 2);
      z[0] = z4.x, z[1] = z4.y, z[2] = z4.z, z[3] = z4.w;
      ri[0] = i4.x, ri[1] = i4.y, ri[2] = i4.z, ri[3] = i4.w;
      zx[0] = za.x, zy[0] = za.y, zx[1] = za.z, zy[1] = za.w, zx[2] = zb.x, zy[2] = zb.y, zx[3] = zb.z, zy[3] = zb.w;
      const int v = p0 / R.w, u0 = p0 - v * R.w;
#pragma unroll
      for (int k = 0; k < kLanePixels; ++k) tx[k] = R.tx[u0 + k];
      ty = R.ty[v];
    }
    int cls[kLanePixels];
    float dist[kLanePixels];
    residual_mask_pixels<kLanePixels>(d, kt, R.P, R.max_distance, z, zx, zy, ri, tx, ty, cls, dist);
    unsigned cnt[kCnt] = {0u, 0u, 0u, 0u, 0u, 0u};
    unsigned word = 0u, last = 0u;
#pragma unroll
    for (int k = 0; k < kLanePixels; ++k) {
      const int c = live ? cls[k] : -2;  // -2: no pixel
      const bool keep = c == (int)kRmInlier || (c == (int)kRmInvalid && R.invalid_keep != 0) || (c == -1 && R.unevaluated_keep != 0);
      word |= keep ? (1u << (8 * k)) : 0u;
      last = c >= 0 ? (unsigned)(p0 + k + 1) : last;
      cnt[kRmEvaluated] += (unsigned)__popcll(__ballot(c >= 0));
      cnt[kRmInvalid] += (unsigned)__popcll(__ballot(c == (int)kRmInvalid));
      cnt[kRmInlier] += (unsigned)__popcll(__ballot(c == (int)kRmInlier));
      cnt[kRmOutlier] += (unsigned)__popcll(__ballot(c == (int)kRmOutlier));
      cnt[4] += (unsigned)__popcll(__ballot(keep));
    }
    if (live) {
      *(unsigned *)(R.out + p0) = word;
      if (R.distance) *(float4 *)(R.distance + p0) = make_float4(dist[0], dist[1], dist[2], dist[3]);
    }
#pragma unroll
    for (int m = kWave / 2; m >= 1; m >>= 1) {  // the wave's last evaluated pixel
      const unsigned o = (unsigned)__shfl_xor((int)last, m, kWave);
      last = o > last ? o : last;
    }
    cnt[5] = last;
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < kCnt; ++c) s_cnt[wave][c] = cnt[c];
    }
    __syncthreads();
    if (threadIdx.x < kCnt) {
      unsigned sum = 0u;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum = threadIdx.x == 5 ? (s_cnt[w][5] > sum ? s_cnt[w][5] : sum) : sum + s_cnt[w][threadIdx.x];
      if (sum) {
        if (threadIdx.x < 4) atomicAdd(R.counts + threadIdx.x, sum);
        else if (threadIdx.x == 4) atomicAdd(R.kept, (int)sum);
        else atomicMax(R.counts + kRmLast, sum);
      }
    }
    // this block is done with the record: every wave's stores and atomics have completed, then one lane publishes them and counts
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // (also: s_cnt may be written again for the block's next record)
    if (threadIdx.x == 0) {
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      const unsigned n_blocks = (unsigned)((R.n + kResidualMaskChunk - 1) / kResidualMaskChunk);
      const unsigned drawn = __hip_atomic_fetch_add(R.counts + kRmDone, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (drawn == n_blocks - 1u) {  // the level is complete: Q3
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        const unsigned n_eval = __hip_atomic_load(R.counts + kRmEvaluated, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const unsigned last1 = __hip_atomic_load(R.counts + kRmLast, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((n_eval & 1u) && last1 >= 1u && last1 <= (unsigned)R.n) {
          const int q = (int)last1 - 1, v = q / R.w, u = q - v * R.w;
          const float2 zd = R.zd[q];
          const float qz[1] = {R.z[q]}, qzx[1] = {zd.x}, qzy[1] = {zd.y}, qri[1] = {R.ri[q]}, qtx[1] = {R.tx[u]};
          int qcls[1];
          float qd[1];
          residual_mask_pixels<1>(d, kt, R.P, R.max_distance, qz, qzx, qzy, qri, qtx, R.ty[v], qcls, qd);
          if (qcls[0] == (int)kRmInlier || qcls[0] == (int)kRmOutlier) {
            atomicSub(R.counts + qcls[0], 1u);
            atomicAdd(R.counts + kRmInvalid, 1u);
            const int was = qcls[0] == (int)kRmInlier ? 1 : 0, now = R.invalid_keep != 0 ? 1 : 0;
            if (now != was) atomicAdd(R.kept, now - was);
            R.out[q] = (unsigned char)now;
            if (R.distance) R.distance[q] = qnan;
          }
        }
      }
    }
  }
}

hipError_t launch_residual_mask(const ResidualMaskRecord *records, int n_records, int max_n, hipStream_t stream) {
  LaunchGuard guard;
  const unsigned gx = (unsigned)((max_n + kResidualMaskChunk - 1) / kResidualMaskChunk);
  const unsigned gy = host::grid_rows(n_records, gx, kResidualMaskBlock);  // a block takes further records in steps of gridDim.y
  hipLaunchKernelGGL(k_residual_mask, dim3(gx, gy), dim3(kResidualMaskBlock), 0, stream, records, n_records);
  return hipGetLastError();
}

// ---- pose scoring (dvo_amd_score_poses, dvo_pose_score.cpp; the rule is pinned in include/dvo_amd.h under "Pose scoring") ---------
// k_score_q3: one block per (reference, level) of a call.  What Q3 takes out of a level -- the last evaluated pixel, if their
// number is odd -- depends on the reference alone, not on the pose: it is found once, ahead of the scoring kernel on the same
// stream, and k_score_poses reads it as an index.  There is no hand-off between blocks anywhere in this feature.
__global__ void __launch_bounds__(kResidualMaskBlock) k_score_q3(PoseScoreLevel *__restrict__ levels) {
  constexpr int kWaves = kResidualMaskBlock / kWave;
  __shared__ int s_cnt[kWaves], s_last[kWaves];
  PoseScoreLevel &L = levels[blockIdx.x];
  const int n = L.n;
  const float *z = L.z;
  const float2 *zd = L.zd;
  int cnt = 0, last = -1;
  for (int i = threadIdx.x; i < n; i += kResidualMaskBlock) {  // (i grows: the last hit of a lane is its largest)
    const float zi = z[i];
    const float2 g = zd[i];
    const bool evaluated = (zi == zi) && (g.x == g.x) && (g.y == g.y);
    cnt += evaluated ? 1 : 0;
    last = evaluated ? i : last;
  }
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) {
    cnt += __shfl_xor(cnt, m, kWave);
    const int o = __shfl_xor(last, m, kWave);
    last = o > last ? o : last;
  }
  if ((threadIdx.x & (kWave - 1)) == 0) s_cnt[threadIdx.x >> 6] = cnt, s_last[threadIdx.x >> 6] = last;
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0, l = -1;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) c += s_cnt[w], l = s_last[w] > l ? s_last[w] : l;
    L.q3 = (c & 1) ? l : -1;
  }
}

// k_score_poses: ONE launch over all (pair, hypothesis tile) items of a call.  blockIdx.x is a chunk of the reference level as in
// k_residual_mask, blockIdx.y strides over the items.  A lane loads its four pixels once and keeps them in registers; per
// hypothesis only the twelve floats of K T change, read through the constant address space (wave-uniform: scalar registers), and
// residual_mask_pixels<4> -- k_residual_mask's residual stage and verdict, rounding-mode fencing included -- runs on the same
// registers again.  Every sum is an integer: counts by ballots, the wave's cost in 32 bits (a lane adds four q <= 2^20, a wave at
// most 2^28, a block 2^30), per wave into LDS, and one 64-bit atomic per non-zero sum per (block, hypothesis) at the tile's end.
__global__ void __launch_bounds__(kResidualMaskBlock) k_score_poses(const PoseScoreRecord *__restrict__ records,
                                                                    const int2 *__restrict__ items, int n_items) {
  constexpr int kWaves = kResidualMaskBlock / kWave, kLanePixels = kResidualMaskLanePixels;
  static_assert(kPoseScoreTile * kPsWords <= kResidualMaskBlock, "one lane per (hypothesis, sum) of a tile");
  __shared__ unsigned s_sum[kWaves][kPoseScoreTile][kPsWords];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  for (int it = blockIdx.y; it < n_items; it += gridDim.y) {
    const int2 item = items[it];  // uniform over the block
    const PoseScoreRecord R = records[item.x];
    if (blockIdx.x * kResidualMaskChunk >= R.n) continue;  // (block-uniform)
    const LevelPairDesc d = residual_mask_desc(R.cur);
    const int p0 = (blockIdx.x * kResidualMaskBlock + threadIdx.x) * kLanePixels;
    const bool live = p0 < R.n;  // (n is a multiple of 4: four pixels or none, all in one row)
    const float qnan = u2f(0x7fc00000u);
    float z[kLanePixels] = {qnan, qnan, qnan, qnan}, zx[kLanePixels] = {qnan, qnan, qnan, qnan}, zy[kLanePixels] = {qnan, qnan, qnan, qnan};
    float ri[kLanePixels] = {0.f, 0.f, 0.f, 0.f}, tx[kLanePixels] = {0.f, 0.f, 0.f, 0.f};
    float ty = 0.f;
    if (live) {
      const float4 z4 = *(const float4 *)(R.z + p0), i4 = *(const float4 *)(R.ri + p0);
      const float4 za = *(const float4 *)(R.zd + p0), zb = *(const float4 *)(R.zd + p0 + 2);
      z[0] = z4.x, z[1] = z4.y, z[2] = z4.z, z[3] = z4.w;
      ri[0] = i4.x, ri[1] = i4.y, ri[2] = i4.z, ri[3] = i4.w;
      zx[0] = za.x, zy[0] = za.y, zx[1] = za.z, zy[1] = za.w, zx[2] = zb.x, zy[2] = zb.y, zx[3] = zb.z, zy[3] = zb.w;
      const int v = p0 / R.w, u0 = p0 - v * R.w;
#pragma unroll
      for (int k = 0; k < kLanePixels; ++k) tx[k] = R.tx[u0 + k];
      ty = R.ty[v];
    }
    const int q3 = R.level->q3;  // (written by k_score_q3, a launch earlier on this stream)
    const int j0 = item.y, j1 = j0 + kPoseScoreTile < R.m ? j0 + kPoseScoreTile : R.m;
    for (int j = j0; j < j1; ++j) {
      const DVO_CONST float *ktc = (const DVO_CONST float *)(R.kt + 12 * (size_t)j);
      float kt[12];
#pragma unroll
      for (int i = 0; i < 12; ++i) kt[i] = ktc[i];
      int cls[kLanePixels];
      float dist[kLanePixels];
      residual_mask_pixels<kLanePixels>(d, kt, R.P, R.max_distance, z, zx, zy, ri, tx, ty, cls, dist);  // (no pixel: z NaN, unevaluated)
      unsigned n_invalid = 0u, n_inlier = 0u, n_outlier = 0u, cost = 0u;
#pragma unroll
      for (int k = 0; k < kLanePixels; ++k) {
        const int c = (cls[k] >= 0 && p0 + k == q3) ? (int)kRmInvalid : cls[k];  // Q3
        n_invalid += (unsigned)__popcll(__ballot(c == (int)kRmInvalid));
        n_inlier += (unsigned)__popcll(__ballot(c == (int)kRmInlier));
        n_outlier += (unsigned)__popcll(__ballot(c == (int)kRmOutlier));
        // q(d) = floor(d * 1024): the product is exact (a power of two, d <= max_distance <= 1024); a negative d -- a precision
        // that is not positive semidefinite -- costs 0
        const unsigned q = (unsigned)__builtin_floorf(__builtin_fmaxf(dist[k], 0.0f) * 1024.0f);
        cost += c == (int)kRmInlier ? q : c == (int)kRmOutlier ? R.q_max : 0u;
      }
#pragma unroll
      for (int m = kWave / 2; m >= 1; m >>= 1) cost += (unsigned)__shfl_xor((int)cost, m, kWave);
      if (lane == 0) {
        unsigned *s = s_sum[wave][j - j0];
        s[kPsInvalid] = n_invalid, s[kPsInlier] = n_inlier, s[kPsOutlier] = n_outlier, s[kPsCost] = cost;
      }
    }
    __syncthreads();
    if ((int)threadIdx.x < (j1 - j0) * kPsWords) {
      const int jj = threadIdx.x / kPsWords, q = threadIdx.x % kPsWords;
      unsigned sum = 0u;
#pragma unroll
      for (int w = 0; w < kWaves; ++w) sum += s_sum[w][jj][q];
      if (sum) atomicAdd(R.sums + (size_t)(j0 + jj) * kPsWords + q, (unsigned long long)sum);
    }
    __syncthreads();  // (s_sum is written again for the block's next item)
  }
}

hipError_t launch_score_poses(PoseScoreLevel *levels, int n_levels, const PoseScoreRecord *records, const int2 *items, int n_items,
                              int max_n, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_score_q3, dim3((unsigned)n_levels), dim3(kResidualMaskBlock), 0, stream, levels);
  const unsigned gx = (unsigned)((max_n + kResidualMaskChunk - 1) / kResidualMaskChunk);
  const unsigned gy = host::grid_rows(n_items, gx, kResidualMaskBlock);  // a block takes further items in steps of gridDim.y
  hipLaunchKernelGGL(k_score_poses, dim3(gx, gy), dim3(kResidualMaskBlock), 0, stream, records, items, n_items);
  return hipGetLastError();
}

// The selected pixels of a level in scan order, compacted (round 5, end): what the residual pass walks.  The reference compacts
// too -- PointSelection::select fills a dense array of the selected points (point_selection.cpp:119-152) and computeResidualsSse
// walks that array -- so the pass's cost follows the selection, not the image.  One exclusive prefix over k_select's per-block
// counts (one block), then every 256-pixel block writes its selected pixels behind the blocks before it: depth, intensity and its
// derivatives, the pixel's ray (tx[column], ty[row]: the residual pass no longer tracks rows and columns) and the pixel index (the
// debug entries scatter per-point results back to the image with it).  Entries from the even point count (Q3, see
// k_select_finish) up to n_pad are padding: depth NaN, everything else zero.
__global__ __launch_bounds__(256) void k_select_prefix(const int2 *__restrict__ block_partials, int n_blocks, int *__restrict__ prefix) {
  const int chunk = (n_blocks + 255) / 256;
  const int b0 = (int)threadIdx.x * chunk, b1 = b0 + chunk < n_blocks ? b0 + chunk : n_blocks;
  int c = 0;
  for (int b = b0; b < b1; ++b) c += block_partials[b].x;
  __shared__ int sh[256];
  sh[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) {
      const int v = sh[t];
      sh[t] = run, run += v;
    }
  }
  __syncthreads();
  int run = sh[threadIdx.x];
  for (int b = b0; b < b1; ++b) prefix[b] = run, run += block_partials[b].x;
}

__global__ __launch_bounds__(256) void k_compact(const float *__restrict__ zsel, const float *__restrict__ r_i, const float *__restrict__ r_ix,
                                                 const float *__restrict__ r_iy, const float *__restrict__ tx, const float *__restrict__ ty,
                                                 int w, int n, int n_pad, const int *__restrict__ prefix, const int *__restrict__ counters,
                                                 float *__restrict__ cz, float *__restrict__ ci, float *__restrict__ cix,
                                                 float *__restrict__ ciy, float *__restrict__ ctx, float *__restrict__ cty,
                                                 int *__restrict__ cpix) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n_pts = counters[0] & ~1;  // Q3: an odd trailing point is never looked at (its zsel entry is NaN already)
  const float z = i < n ? zsel[i] : u2f(0x7fc00000u);
  const bool ok = z == z;
  const unsigned long long m = __ballot(ok);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  __shared__ int sh_cnt[4];
  if (lane == 0) sh_cnt[wave] = __popcll(m);
  __syncthreads();
  int before = prefix[blockIdx.x];
  for (int k = 0; k < wave; ++k) before += sh_cnt[k];
  if (ok) {
    const int p = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    const int row = i / w, col = i - row * w;
    cz[p] = z, ci[p] = r_i[i], cix[p] = r_ix[i], ciy[p] = r_iy[i], ctx[p] = tx[col], cty[p] = ty[row], cpix[p] = i;
  }
  if (i >= n_pts && i < n_pad) cz[i] = u2f(0x7fc00000u), ci[i] = 0.0f, cix[i] = 0.0f, ciy[i] = 0.0f, ctx[i] = 0.0f, cty[i] = 0.0f, cpix[i] = -1;
}

hipError_t launch_compact(const float *zsel, const float *r_i, const float *r_ix, const float *r_iy, const float *tx, const float *ty, int w,
                          int n, int n_pad, const int2 *block_partials, int *prefix, const int *counters, float *cz, float *ci, float *cix,
                          float *ciy, float *ctx, float *cty, int *cpix, hipStream_t stream) {
  LaunchGuard guard;
  const int n_blocks = (n_pad + 255) / 256;
  hipLaunchKernelGGL(k_select_prefix, dim3(1), dim3(256), 0, stream, block_partials, n_blocks, prefix);
  hipLaunchKernelGGL(k_compact, dim3((unsigned)n_blocks), dim3(256), 0, stream, zsel, r_i, r_ix, r_iy, tx, ty, w, n, n_pad,
                     (const int *)prefix, counters, cz, ci, cix, ciy, ctx, cty, cpix);
  return hipGetLastError();
}

__global__ void k_copy_strided(const float *__restrict__ src, int stride, float *__restrict__ dst, int w, int h) {
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x < w && y < h) dst[(size_t)y * w + x] = src[(size_t)y * stride + x];
}

hipError_t launch_copy_strided(const float *src, int stride, float *dst, int w, int h, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_copy_strided, dim3((unsigned)((w + 255) / 256), (unsigned)h), dim3(256), 0, stream, src, stride, dst, w,
                     h);
  return hipGetLastError();
}

// Frame ingest: raw sensor frame -> the two float base planes of level 0.
//   depth: 0 -> NaN, else (float)raw * scale           (SurfacePyramid::convertRawDepthImageSse, surface_pyramid.cpp:65-105)
//   gray : (B*1868 + G*9617 + R*4899 + 2^13) >> 14      (cv::cvtColor(CV_BGR2GRAY) 8-bit rule + convertTo(CV_32F),
//          or the byte itself for 1-channel input        benchmark_slam.cpp:60-68, camera_dense_tracking.cpp:219-229)
// One thread converts 4 consecutive pixels of a row (level widths are multiples of 4): 12 + 8 bytes in, 2 x 16 bytes out.
// kDepth = false writes the intensity plane alone (the registered ingest fills the depth plane by its own rule, dvo_register.cpp).
template <bool kDepth>
__global__ void k_ingest(const unsigned char *__restrict__ img, int channels, int img_stride_bytes,
                         const unsigned short *__restrict__ raw_z, int z_stride, float z_scale, float *__restrict__ i_plane,
                         float *__restrict__ z_plane, int w, int h) {
  const int x4 = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
  if (x4 * 4 >= w || y >= h) return;
  const unsigned char *ip = img + (size_t)y * img_stride_bytes + (size_t)x4 * 4 * channels;
  unsigned char px[12];
  const int nb = 4 * channels;
  if ((((size_t)ip) & 3) == 0) {
    const unsigned *ip4 = (const unsigned *)ip;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < channels) {
        const unsigned v = ip4[k];
        px[4 * k] = (unsigned char)v, px[4 * k + 1] = (unsigned char)(v >> 8), px[4 * k + 2] = (unsigned char)(v >> 16),
               px[4 * k + 3] = (unsigned char)(v >> 24);
      }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < nb) px[k] = ip[k];
  }
  float g[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (channels == 3) {
      const int b = px[3 * k], gg = px[3 * k + 1], r = px[3 * k + 2];
      g[k] = (float)((b * 1868 + gg * 9617 + r * 4899 + (1 << 13)) >> 14);
    } else {
      g[k] = (float)px[k];
    }
  }
  const size_t o = (size_t)y * w + (size_t)x4 * 4;
  if (!kDepth) {
    *(float4 *)(i_plane + o) = make_float4(g[0], g[1], g[2], g[3]);
    return;
  }
  const unsigned short *zp = raw_z + (size_t)y * z_stride + (size_t)x4 * 4;
  unsigned short zr[4];
  if ((((size_t)zp) & 7) == 0) {
    const uint2 v = *(const uint2 *)zp;
    zr[0] = (unsigned short)v.x, zr[1] = (unsigned short)(v.x >> 16), zr[2] = (unsigned short)v.y,
    zr[3] = (unsigned short)(v.y >> 16);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) zr[k] = zp[k];
  }
  float z[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) z[k] = zr[k] == 0 ? __builtin_nanf("") : (float)zr[k] * z_scale;
  *(float4 *)(i_plane + o) = make_float4(g[0], g[1], g[2], g[3]);
  *(float4 *)(z_plane + o) = make_float4(z[0], z[1], z[2], z[3]);
}

hipError_t launch_ingest(const unsigned char *img, int channels, int img_stride_bytes, const unsigned short *raw_z,
                         int z_stride, float z_scale, float *i_plane, float *z_plane, int w, int h, hipStream_t stream) {
  LaunchGuard guard;
  const int wq = w / 4;
  hipLaunchKernelGGL(k_ingest<true>, dim3((unsigned)((wq + 63) / 64), (unsigned)h), dim3(64), 0, stream, img, channels,
                     img_stride_bytes, raw_z, z_stride, z_scale, i_plane, z_plane, w, h);
  return hipGetLastError();
}

hipError_t launch_ingest_intensity(const unsigned char *img, int channels, int img_stride_bytes, float *i_plane, int w, int h,
                                   hipStream_t stream) {
  LaunchGuard guard;
  const int wq = w / 4;
  hipLaunchKernelGGL(k_ingest<false>, dim3((unsigned)((wq + 63) / 64), (unsigned)h), dim3(64), 0, stream, img, channels,
                     img_stride_bytes, (const unsigned short *)nullptr, 0, 0.0f, i_plane, (float *)nullptr, w, h);
  return hipGetLastError();
}

__global__ void k_mask_from_zsel(const float *__restrict__ zsel, int n, int last_dropped, unsigned char *__restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mask[i] = (zsel[i] == zsel[i] || i == last_dropped) ? 1 : 0;
}

hipError_t launch_mask_from_zsel(const float *zsel, int n, int last_dropped, unsigned char *mask, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_mask_from_zsel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, zsel, n, last_dropped, mask);
  return hipGetLastError();
}

__global__ void k_unpack_plane(const float4 *__restrict__ c_a, const float2 *__restrict__ c_b, int plane, int n,
                               float *__restrict__ dst) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float v;
  switch (plane) {
    case 0: v = c_a[i].x; break;
    case 1: v = c_a[i].y; break;
    case 2: v = c_a[i].z; break;
    case 3: v = c_a[i].w; break;
    case 4: v = c_b[i].x; break;
    default: v = c_b[i].y; break;
  }
  dst[i] = v;
}

hipError_t launch_unpack_plane(const float4 *c_a, const float2 *c_b, int plane, int n, float *dst, hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_unpack_plane, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, c_a, c_b, plane, n, dst);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------------------------
// pyramid construction, N frames per launch (dvo_amd_pyramid_create_raw_batch)
// ------------------------------------------------------------------------------------------------------------------
// The kernels above with the frame as the grid's y dimension: a frame is a row of the BatchFrame table, a level a set of offsets
// from the frame's slab (BatchLevel).  What a pixel's thread computes -- every operation, its order, its rounding, the padding
// values -- is the single-frame kernel's, statement for statement, so a batched pyramid is the singly built one bit for bit.
// Only the tiling differs: these are streaming kernels, so a thread takes the i-th pixel (or group of four) of the whole
// level in scan order instead of the x-th of row blockIdx.y, and no lane idles at a row's end (of the three 64-thread blocks
// k_ingest gives a 640-pixel row the third is half empty, and k_pyr_down's one 256-thread block of an 80-pixel row holds 80
// pixels; here every block but a frame's last is full).  Consecutive lanes still touch consecutive addresses.  The two
// single-block kernels of the selection become one block per frame.

constexpr unsigned kBatchGridFrames = 65535;  // gridDim.y's limit: a launcher splits a larger batch

template <typename T>
__device__ __forceinline__ T *batch_at(const BatchFrame &f, size_t offset) {
  return (T *)(f.slab + offset);
}

// k_ingest<true>
__global__ __launch_bounds__(256) void k_ingest_batch(const BatchFrame *__restrict__ frames, int frame0, int channels,
                                                      int img_stride_bytes, int z_stride, float z_scale, size_t off_i, size_t off_z,
                                                      int w, int h) {
  const int q = blockIdx.x * blockDim.x + threadIdx.x, wq = w / 4;
  if (q >= wq * h) return;
  const int y = q / wq, x4 = q - y * wq;
  const BatchFrame f = frames[frame0 + blockIdx.y];
  float *__restrict__ i_plane = batch_at<float>(f, off_i), *__restrict__ z_plane = batch_at<float>(f, off_z);
  const unsigned char *ip = f.img + (size_t)y * img_stride_bytes + (size_t)x4 * 4 * channels;
  unsigned char px[12];
  const int nb = 4 * channels;
  if ((((size_t)ip) & 3) == 0) {
    const unsigned *ip4 = (const unsigned *)ip;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (k < channels) {
        const unsigned v = ip4[k];
        px[4 * k] = (unsigned char)v, px[4 * k + 1] = (unsigned char)(v >> 8), px[4 * k + 2] = (unsigned char)(v >> 16),
               px[4 * k + 3] = (unsigned char)(v >> 24);
      }
  } else {
#pragma unroll
    for (int k = 0; k < 12; ++k)
      if (k < nb) px[k] = ip[k];
  }
  float g[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (channels == 3) {
      const int b = px[3 * k], gg = px[3 * k + 1], r = px[3 * k + 2];
      g[k] = (float)((b * 1868 + gg * 9617 + r * 4899 + (1 << 13)) >> 14);
    } else {
      g[k] = (float)px[k];
    }
  }
  const size_t o = (size_t)y * w + (size_t)x4 * 4;
  const unsigned short *zp = f.z + (size_t)y * z_stride + (size_t)x4 * 4;
  unsigned short zr[4];
  if ((((size_t)zp) & 7) == 0) {
    const uint2 v = *(const uint2 *)zp;
    zr[0] = (unsigned short)v.x, zr[1] = (unsigned short)(v.x >> 16), zr[2] = (unsigned short)v.y,
    zr[3] = (unsigned short)(v.y >> 16);
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) zr[k] = zp[k];
  }
  float z[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) z[k] = zr[k] == 0 ? __builtin_nanf("") : (float)zr[k] * z_scale;
  *(float4 *)(i_plane + o) = make_float4(g[0], g[1], g[2], g[3]);
  *(float4 *)(z_plane + o) = make_float4(z[0], z[1], z[2], z[3]);
}

// k_pyr_down
__global__ __launch_bounds__(256) void k_pyr_down_batch(const BatchFrame *__restrict__ frames, int frame0, size_t off_ip, size_t off_zp,
                                                        int wp, size_t off_io, size_t off_zo, int w, int h) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= w * h) return;
  const int y = i / w, x = i - y * w;
  const BatchFrame f = frames[frame0 + blockIdx.y];
  const float *__restrict__ ip = batch_at<const float>(f, off_ip), *__restrict__ zp = batch_at<const float>(f, off_zp);
  float *__restrict__ io = batch_at<float>(f, off_io), *__restrict__ zo = batch_at<float>(f, off_zo);
  const float *r0 = ip + (size_t)(2 * y) * wp + 2 * x;
  const float *r1 = r0 + wp;
  io[(size_t)y * w + x] = (((r0[0] + r0[1]) + r1[0]) + r1[1]) / 4.0f;
  zo[(size_t)y * w + x] = zp[(size_t)(2 * y) * wp + 2 * x];
}

// k_level_planes
__global__ __launch_bounds__(256) void k_level_planes_batch(const BatchFrame *__restrict__ frames, int frame0, BatchLevel L) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int w = L.w, h = L.h, n = L.n;
  const float fx = L.fx, fy = L.fy, ox = L.ox, oy = L.oy;
  const BatchFrame f = frames[frame0 + blockIdx.y];
  const float *__restrict__ ip = batch_at<const float>(f, L.i_plane), *__restrict__ zp = batch_at<const float>(f, L.z_plane);
  float4 *__restrict__ c_a = batch_at<float4>(f, L.c_a);
  float2 *__restrict__ c_b = batch_at<float2>(f, L.c_b);
  float *__restrict__ r_i = batch_at<float>(f, L.r_i), *__restrict__ r_ix = batch_at<float>(f, L.r_ix),
                     *__restrict__ r_iy = batch_at<float>(f, L.r_iy);
  float *__restrict__ tx = batch_at<float>(f, L.tx), *__restrict__ ty = batch_at<float>(f, L.ty);
  if (i < w) tx[i] = ((float)i - ox) / fx;
  if (i < h) ty[i] = ((float)i - oy) / fy;
  if (i >= L.n_pad) return;
  if (i >= n) {
    r_i[i] = 0.0f, r_ix[i] = 0.0f, r_iy[i] = 0.0f;
    return;
  }
  const int y = i / w, x = i - y * w;
  const int xp = x > 0 ? x - 1 : 0, xn = x < w - 1 ? x + 1 : w - 1;
  const int yp = y > 0 ? y - 1 : 0, yn = y < h - 1 ? y + 1 : h - 1;
  const float I = ip[i], Z = zp[i];
  const float Ix = (ip[y * w + xn] - ip[y * w + xp]) * 0.5f;
  const float Iy = (ip[yn * w + x] - ip[yp * w + x]) * 0.5f;
  const float Zx = (zp[y * w + xn] - zp[y * w + xp]) * 0.5f;
  const float Zy = (zp[yn * w + x] - zp[yp * w + x]) * 0.5f;
  c_a[i] = make_float4(I, Z, Ix, Iy);
  c_b[i] = make_float2(Zx, Zy);
  r_i[i] = I, r_ix[i] = Ix, r_iy[i] = Iy;
}

// One block per frame, one thread per level: the frame's level descriptors (what pyramid_build and pyramid_selection copy from
// the host, one small copy per pyramid) from the call's one set, whose pointers are offsets from a slab's base.
__global__ __launch_bounds__(64) void k_batch_descs(const BatchFrame *__restrict__ frames, int frame0, BatchDescs D) {
  const int l = threadIdx.x;
  if (l >= D.levels) return;
  const BatchFrame f = frames[frame0 + blockIdx.x];
  CurLevelDesc c = D.cur[l];
  c.c_a = batch_at<const float4>(f, (size_t)c.c_a), c.c_b = batch_at<const float2>(f, (size_t)c.c_b);
  ((CurLevelDesc *)f.desc)[l] = c;
  if (!D.with_ref) return;
  RefLevelDesc r = D.ref[l];
  r.r_zsel = batch_at<const float>(f, (size_t)r.r_zsel);
  r.r_i = batch_at<const float>(f, (size_t)r.r_i), r.r_ix = batch_at<const float>(f, (size_t)r.r_ix),
  r.r_iy = batch_at<const float>(f, (size_t)r.r_iy);
  r.tx = batch_at<const float>(f, (size_t)r.tx), r.ty = batch_at<const float>(f, (size_t)r.ty);
  ((RefLevelDesc *)(f.desc + D.ref_offset))[l] = r;
}

// k_select
__global__ __launch_bounds__(256) void k_select_batch(const BatchFrame *__restrict__ frames, int frame0, size_t off_z, size_t off_ca,
                                                      size_t off_cb, int n, int n_pad, float ti, float td, size_t off_zsel,
                                                      size_t off_partials) {
  const BatchFrame f = frames[frame0 + blockIdx.y];
  const float *__restrict__ zp = batch_at<const float>(f, off_z);
  const float4 *__restrict__ c_a = batch_at<const float4>(f, off_ca);
  const float2 *__restrict__ c_b = batch_at<const float2>(f, off_cb);
  float *__restrict__ zsel = batch_at<float>(f, off_zsel);
  int2 *__restrict__ block_partials = batch_at<int2>(f, off_partials);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  float out = u2f(0x7fc00000u);
  bool ok = false;
  if (i < n) {
    const float z = zp[i];
    const float4 a = c_a[i];
    const float2 b = c_b[i];
    ok = (z == z) && (b.x == b.x) && (b.y == b.y) &&
         (__builtin_fabsf(a.z) > ti || __builtin_fabsf(a.w) > ti || __builtin_fabsf(b.x) > td || __builtin_fabsf(b.y) > td);
    if (ok) out = z;
  }
  if (i < n_pad) zsel[i] = out;
  __shared__ int sh_cnt[4], sh_last[4];
  const unsigned long long m = __ballot(ok);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  if (lane == 0) {
    sh_cnt[wave] = __popcll(m);
    sh_last[wave] = m ? (int)(blockIdx.x * blockDim.x) + wave * kWave + (63 - __builtin_clzll(m)) : -1;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int c = 0, last = -1;
    for (int w = 0; w < 4; ++w) c += sh_cnt[w], last = sh_last[w] > last ? sh_last[w] : last;
    block_partials[blockIdx.x] = make_int2(c, last);
  }
}

// k_select_finish, one block per frame; the two counters go to the pyramid's own slab (k_compact_batch reads them there) and to
// the call's table, from where one copy takes every frame's to the host
__global__ __launch_bounds__(256) void k_select_finish_batch(const BatchFrame *__restrict__ frames, int frame0, size_t off_partials,
                                                             int n_blocks, size_t off_zsel, size_t off_counters,
                                                             int *__restrict__ all_counters, int level, int levels) {
  const int fi = frame0 + blockIdx.x;
  const BatchFrame f = frames[fi];
  const int2 *__restrict__ block_partials = batch_at<const int2>(f, off_partials);
  float *zsel = batch_at<float>(f, off_zsel);
  int *__restrict__ counters = batch_at<int>(f, off_counters);
  int c = 0, last = -1;
  for (int b = threadIdx.x; b < n_blocks; b += 256) {
    const int2 p = block_partials[b];
    c += p.x, last = p.y > last ? p.y : last;
  }
  __shared__ int sh_c[256], sh_l[256];
  sh_c[threadIdx.x] = c, sh_l[threadIdx.x] = last;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) {
      sh_c[threadIdx.x] += sh_c[threadIdx.x + s];
      sh_l[threadIdx.x] = sh_l[threadIdx.x + s] > sh_l[threadIdx.x] ? sh_l[threadIdx.x + s] : sh_l[threadIdx.x];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    counters[0] = sh_c[0], counters[1] = sh_l[0];
    int *mine = all_counters + 2 * ((size_t)fi * levels + level);
    mine[0] = sh_c[0], mine[1] = sh_l[0];
    if ((sh_c[0] & 1) && sh_l[0] >= 0) zsel[sh_l[0]] = u2f(0x7fc00000u);
  }
}

// k_select_prefix, one block per frame
__global__ __launch_bounds__(256) void k_select_prefix_batch(const BatchFrame *__restrict__ frames, int frame0, size_t off_partials,
                                                             int n_blocks, size_t off_prefix) {
  const BatchFrame f = frames[frame0 + blockIdx.x];
  const int2 *__restrict__ block_partials = batch_at<const int2>(f, off_partials);
  int *__restrict__ prefix = batch_at<int>(f, off_prefix);
  const int chunk = (n_blocks + 255) / 256;
  const int b0 = (int)threadIdx.x * chunk, b1 = b0 + chunk < n_blocks ? b0 + chunk : n_blocks;
  int c = 0;
  for (int b = b0; b < b1; ++b) c += block_partials[b].x;
  __shared__ int sh[256];
  sh[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < 256; ++t) {
      const int v = sh[t];
      sh[t] = run, run += v;
    }
  }
  __syncthreads();
  int run = sh[threadIdx.x];
  for (int b = b0; b < b1; ++b) prefix[b] = run, run += block_partials[b].x;
}

// k_compact
__global__ __launch_bounds__(256) void k_compact_batch(const BatchFrame *__restrict__ frames, int frame0, BatchLevel L) {
  const BatchFrame f = frames[frame0 + blockIdx.y];
  const float *__restrict__ zsel = batch_at<const float>(f, L.zsel);
  const float *__restrict__ r_i = batch_at<const float>(f, L.r_i), *__restrict__ r_ix = batch_at<const float>(f, L.r_ix),
                           *__restrict__ r_iy = batch_at<const float>(f, L.r_iy);
  const float *__restrict__ tx = batch_at<const float>(f, L.tx), *__restrict__ ty = batch_at<const float>(f, L.ty);
  const int *__restrict__ prefix = batch_at<const int>(f, L.prefix), *__restrict__ counters = batch_at<const int>(f, L.counters);
  float *__restrict__ cz = batch_at<float>(f, L.pts[0]), *__restrict__ ci = batch_at<float>(f, L.pts[1]),
                     *__restrict__ cix = batch_at<float>(f, L.pts[2]), *__restrict__ ciy = batch_at<float>(f, L.pts[3]),
                     *__restrict__ ctx = batch_at<float>(f, L.pts[4]), *__restrict__ cty = batch_at<float>(f, L.pts[5]);
  int *__restrict__ cpix = batch_at<int>(f, L.pts[6]);
  const int w = L.w, n = L.n, n_pad = L.n_pad;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n_pts = counters[0] & ~1;  // Q3: an odd trailing point is never looked at (its zsel entry is NaN already)
  const float z = i < n ? zsel[i] : u2f(0x7fc00000u);
  const bool ok = z == z;
  const unsigned long long m = __ballot(ok);
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
  __shared__ int sh_cnt[4];
  if (lane == 0) sh_cnt[wave] = __popcll(m);
  __syncthreads();
  int before = prefix[blockIdx.x];
  for (int k = 0; k < wave; ++k) before += sh_cnt[k];
  if (ok) {
    const int p = before + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
    const int row = i / w, col = i - row * w;
    cz[p] = z, ci[p] = r_i[i], cix[p] = r_ix[i], ciy[p] = r_iy[i], ctx[p] = tx[col], cty[p] = ty[row], cpix[p] = i;
  }
  if (i >= n_pts && i < n_pad) cz[i] = u2f(0x7fc00000u), ci[i] = 0.0f, cix[i] = 0.0f, ciy[i] = 0.0f, ctx[i] = 0.0f, cty[i] = 0.0f, cpix[i] = -1;
}

// frames [0, count) in launches of at most kBatchGridFrames each: launch(first frame, frames of this launch)
template <typename F>
static hipError_t batch_launches(int count, int *launches, F launch) {
  LaunchGuard guard;
  for (int f0 = 0; f0 < count; f0 += (int)kBatchGridFrames) {
    const int nf = count - f0 < (int)kBatchGridFrames ? count - f0 : (int)kBatchGridFrames;
    launch(f0, (unsigned)nf);
    *launches += 1;
  }
  return hipGetLastError();
}

static unsigned blocks256(long long n) { return (unsigned)((n + 255) / 256); }

hipError_t launch_ingest_batch(const BatchFrame *frames, int count, int channels, int img_stride_bytes, int z_stride, float z_scale,
                               const BatchLevel &L0, hipStream_t stream, int *launches) {
  return batch_launches(count, launches, [&](int f0, unsigned nf) {
    hipLaunchKernelGGL(k_ingest_batch, dim3(blocks256((long long)(L0.w / 4) * L0.h), nf), dim3(256), 0, stream, frames, f0, channels,
                       img_stride_bytes, z_stride, z_scale, L0.i_plane, L0.z_plane, L0.w, L0.h);
  });
}

hipError_t launch_pyr_down_batch(const BatchFrame *frames, int count, const BatchLevel &prev, const BatchLevel &L, hipStream_t stream,
                                 int *launches) {
  return batch_launches(count, launches, [&](int f0, unsigned nf) {
    hipLaunchKernelGGL(k_pyr_down_batch, dim3(blocks256(L.n), nf), dim3(256), 0, stream, frames, f0, prev.i_plane, prev.z_plane, prev.w,
                       L.i_plane, L.z_plane, L.w, L.h);
  });
}

hipError_t launch_level_planes_batch(const BatchFrame *frames, int count, const BatchLevel &L, hipStream_t stream, int *launches) {
  int span = L.n_pad > L.h ? L.n_pad : L.h;
  if (L.w > span) span = L.w;
  return batch_launches(count, launches, [&](int f0, unsigned nf) {
    hipLaunchKernelGGL(k_level_planes_batch, dim3(blocks256(span), nf), dim3(256), 0, stream, frames, f0, L);
  });
}

hipError_t launch_batch_descs(const BatchFrame *frames, int count, const BatchDescs &descs, hipStream_t stream, int *launches) {
  static_assert(kBatchMaxLevels <= 64, "k_batch_descs: one thread per level");
  return batch_launches(count, launches, [&](int f0, unsigned nf) {
    hipLaunchKernelGGL(k_batch_descs, dim3(nf), dim3(64), 0, stream, frames, f0, descs);
  });
}

hipError_t launch_select_batch(const BatchFrame *frames, int count, const BatchLevel &L, float ti, float td, int *all_counters,
                               int level, int levels, hipStream_t stream, int *launches) {
  const int n_blocks = (L.n_pad + 255) / 256;
  hipError_t e = batch_launches(count, launches, [&](int f0, unsigned nf) {
    hipLaunchKernelGGL(k_select_batch, dim3((unsigned)n_blocks, nf), dim3(256), 0, stream, frames, f0, L.z_plane, L.c_a, L.c_b, L.n,
                       L.n_pad, ti, td, L.zsel, L.partials);
  });
  if (e != hipSuccess) return e;
  return batch_launches(count, launches, [&](int f0, unsigned nf) {
    hipLaunchKernelGGL(k_select_finish_batch, dim3(nf), dim3(256), 0, stream, frames, f0, L.partials, n_blocks, L.zsel, L.counters,
                       all_counters, level, levels);
  });
}

hipError_t launch_compact_batch(const BatchFrame *frames, int count, const BatchLevel &L, hipStream_t stream, int *launches) {
  const int n_blocks = (L.n_pad + 255) / 256;
  hipError_t e = batch_launches(count, launches, [&](int f0, unsigned nf) {
    hipLaunchKernelGGL(k_select_prefix_batch, dim3(nf), dim3(256), 0, stream, frames, f0, L.partials, n_blocks, L.prefix);
  });
  if (e != hipSuccess) return e;
  return batch_launches(count, launches, [&](int f0, unsigned nf) {
    hipLaunchKernelGGL(k_compact_batch, dim3((unsigned)n_blocks, nf), dim3(256), 0, stream, frames, f0, L);
  });
}

// ------------------------------------------------------------------------------------------------------------------
// the place index (dvo_amd_place_*, dvo_place.cpp): int8 appearance descriptors, their dot products, the best k per query
// ------------------------------------------------------------------------------------------------------------------
// The rule is pinned in include/dvo_amd.h under "Place index"; tests/place_ref.py restates it.  Everything a kernel below leaves in
// memory is an integer or a double formed from integers by two products in a fixed order: nothing depends on the launch geometry.

// One block per pyramid.  A thread takes four consecutive pixels at a time (dim is a multiple of 64): four int8 values, one
// 32-bit store, the zero padding behind w * h included.  The row's norm is one reduction over the block: no atomics.
__global__ __launch_bounds__(kPlaceBlock) void k_place_describe(const float *const *__restrict__ planes, int w, int h, int dim, float gain,
                                                               signed char *__restrict__ rows, int *__restrict__ nn) {
  __shared__ int s_sum[kPlaceBlock / kWave];
  const float *__restrict__ I = planes[blockIdx.x];
  signed char *__restrict__ row = rows + (size_t)blockIdx.x * (size_t)dim;
  const int n = w * h;
  int sum = 0;
  for (int p0 = (int)threadIdx.x * 4; p0 < dim; p0 += kPlaceBlock * 4) {
    unsigned word = 0u;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int p = p0 + i;
      int q = 0;
      if (p < n) {
        const int v = p / w, u = p - v * w;
        const int v0 = v > 0 ? v - 1 : 0, v1 = v < h - 1 ? v + 1 : h - 1;
        const int u0 = u > 0 ? u - 1 : 0, u1 = u < w - 1 ? u + 1 : w - 1;
        float s = 0.0f;
        for (int y = v0; y <= v1; ++y)
          for (int x = u0; x <= u1; ++x) s = s + I[y * w + x];
        const float c = (float)((v1 - v0 + 1) * (u1 - u0 + 1));
        const float m = s / c;
        const float d = (I[p] - m) * gain;
        if (fabsf(d) <= 3.402823466e38f) q = (int)fminf(127.0f, fmaxf(-127.0f, rintf(d)));  // (false for NaN: q stays 0)
      }
      sum += q * q;
      word |= (unsigned)(q & 0xff) << (8 * i);
    }
    *(unsigned *)(row + p0) = word;  // (p0 + 3 < dim; rows are 64-byte aligned)
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
  if ((threadIdx.x & (kWave - 1)) == 0) s_sum[threadIdx.x / kWave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int total = 0;
#pragma unroll
    for (int k = 0; k < kPlaceBlock / kWave; ++k) total += s_sum[k];
    nn[blockIdx.x] = total;  // <= 65536 * 127 * 127 < 2^31
  }
}

hipError_t launch_place_describe(const float *const *planes, int n, int w, int h, int dim, float gain, signed char *rows, int *nn,
                                 hipStream_t stream) {
  LaunchGuard guard;
  hipLaunchKernelGGL(k_place_describe, dim3((unsigned)n), dim3(kPlaceBlock), 0, stream, planes, w, h, dim, gain, rows, nn);
  return hipGetLastError();
}

// dots = Q . X^T with v_mfma_i32_16x16x64_i8.  A workgroup owns a tile of T x T blocks of 16 queries x 16 keys; its four waves
// split the k-steps of 64 bytes between them (wave s takes steps s, s + 4, ...: integer sums, any order gives the same result) and
// wave 0 adds the other three's partial tiles through LDS and writes.  Both operands are rows contiguous along k: lane l's
// fragment of either is the 16 bytes at [row l & 15][64 * step + 16 * (l >> 4)] -- one 16-byte load -- and because both sides use
// the same lane -> k rule the order of k inside the instruction does not matter to a dot product.  The result block has its key on
// the lane and its queries in the registers: D[query 4 * (l >> 4) + reg][key l & 15].
// A partial tile reads, for the rows it lacks, the last row that exists instead of zeros: an element of D depends on its own
// query row and its own key row alone, so every load is unconditional and in bounds and the elements outside n_queries x n are
// simply not written.
typedef int place_i4 __attribute__((ext_vector_type(4)));

template <int T>
__global__ __launch_bounds__(kPlaceBlock) void k_place_dots(const signed char *__restrict__ index, const int *__restrict__ query_ids,
                                                           const signed char *__restrict__ queries, int n_queries,
                                                           const signed char *__restrict__ keys, int n, int dim, int *__restrict__ dots) {
  constexpr int kWaves = kPlaceBlock / kWave;
  constexpr int kRegs = T * T * 4;  // accumulator registers of a wave
  __shared__ int s_part[(kWaves - 1) * kRegs * kWave];
  const int lane = (int)threadIdx.x & (kWave - 1), wave = (int)threadIdx.x / kWave;
  const int q0 = (int)blockIdx.y * (16 * T), k0 = (int)blockIdx.x * (16 * T);
  const int in_block = lane & 15, at = (lane >> 4) * 16;
  const signed char *a_row[T], *b_row[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int q = min(q0 + 16 * t + in_block, n_queries - 1), j = min(k0 + 16 * t + in_block, n - 1);
    a_row[t] = (query_ids ? index + (size_t)query_ids[q] * (size_t)dim : queries + (size_t)q * (size_t)dim) + at;
    b_row[t] = keys + (size_t)j * (size_t)dim + at;
  }
  place_i4 acc[T][T];
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j) acc[i][j] = place_i4{0, 0, 0, 0};
  const int steps = dim / 64;
  // pipelined by one step: the fragments of the wave's next step are in flight while this step's feed the matrix pipe (behind
  // the wave's last step the same fragments are loaded once more: in bounds, not used)
  place_i4 a[T], b[T];
  {
    const size_t off = (size_t)min(wave, steps - 1) * 64;
#pragma unroll
    for (int t = 0; t < T; ++t) a[t] = *(const place_i4 *)(a_row[t] + off), b[t] = *(const place_i4 *)(b_row[t] + off);
  }
  for (int s = wave; s < steps; s += kWaves) {
    const size_t off = (size_t)(s + kWaves < steps ? s + kWaves : s) * 64;
    place_i4 an[T], bn[T];
#pragma unroll
    for (int t = 0; t < T; ++t) an[t] = *(const place_i4 *)(a_row[t] + off), bn[t] = *(const place_i4 *)(b_row[t] + off);
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < T; ++t) a[t] = an[t], b[t] = bn[t];
  }
  if (wave > 0) {
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
      for (int j = 0; j < T; ++j)
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) s_part[((wave - 1) * kRegs + (i * T + j) * 4 + reg) * kWave + lane] = acc[i][j][reg];
  }
  __syncthreads();
  if (wave > 0) return;
#pragma unroll
  for (int i = 0; i < T; ++i)
#pragma unroll
    for (int j = 0; j < T; ++j) {
      const int key = k0 + 16 * j + in_block;
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        const int q = q0 + 16 * i + 4 * (lane >> 4) + reg;
        int v = acc[i][j][reg];
#pragma unroll
        for (int o = 0; o < kWaves - 1; ++o) v += s_part[(o * kRegs + (i * T + j) * 4 + reg) * kWave + lane];
        if (q < n_queries && key < n) dots[(size_t)q * (size_t)n + (size_t)key] = v;
      }
    }
}

hipError_t launch_place_dots(const signed char *index, const int *query_ids, const signed char *queries, int n_queries,
                             const signed char *keys, int n, int dim, int *dots, int tile, hipStream_t stream) {
  if (n_queries <= 0 || n <= 0) return hipSuccess;
  LaunchGuard guard;
  // the 1 x N query is bound by reading N rows: small tiles spread them over the device; many queries want reuse of a fragment
  if (tile != 1 && tile != 2 && tile != 4) tile = n_queries <= 16 ? 1 : n_queries <= 32 ? 2 : 4;
  const int side = 16 * tile;
  const dim3 grid((unsigned)((n + side - 1) / side), (unsigned)((n_queries + side - 1) / side));
  if (tile == 1)
    hipLaunchKernelGGL(k_place_dots<1>, grid, dim3(kPlaceBlock), 0, stream, index, query_ids, queries, n_queries, keys, n, dim, dots);
  else if (tile == 2)
    hipLaunchKernelGGL(k_place_dots<2>, grid, dim3(kPlaceBlock), 0, stream, index, query_ids, queries, n_queries, keys, n, dim, dots);
  else
    hipLaunchKernelGGL(k_place_dots<4>, grid, dim3(kPlaceBlock), 0, stream, index, query_ids, queries, n_queries, keys, n, dim, dots);
  return hipGetLastError();
}

// One block per query: k rounds of arg-max over the query's row of dots.  The order is (score descending, id ascending), so the
// pick of a round is the best key that comes strictly after the previous pick in that order: nothing is marked, nothing is sorted.
// score = ((double)dot * r_query) * r[j]: two double products, each rounded on its own (no contraction).
__global__ __launch_bounds__(kPlaceBlock) void k_place_topk(const int *__restrict__ dots, int n, const int *__restrict__ query_ids,
                                                           const double *__restrict__ r_query, const double *__restrict__ r, int k,
                                                           double min_score, int exclude_recent, int *__restrict__ candidates,
                                                           double *__restrict__ scores, int *__restrict__ counts) {
  constexpr int kWaves = kPlaceBlock / kWave;
  constexpr int kNone = 0x7fffffff;
  __shared__ double s_score[kWaves];
  __shared__ int s_id[kWaves];
  const int i = (int)blockIdx.x;
  const int *__restrict__ row = dots + (size_t)i * (size_t)n;
  const int qid = query_ids[i];  // < 0: a frame, no key is excluded
  const double rq = r_query[i];
  double prev_score = __builtin_huge_val();
  int prev_id = -1, found = 0;
  for (int round = 0; round < k; ++round) {
    double best = -__builtin_huge_val();
    int best_id = kNone;
    for (int j = (int)threadIdx.x; j < n; j += kPlaceBlock) {
      const int apart = j > qid ? j - qid : qid - j;
      const bool eligible = qid < 0 || apart > exclude_recent;  // (exclude_recent >= 0: the query's own row is never eligible)
      const double s = ((double)row[j] * rq) * r[j];
      const bool after = s < prev_score || (s == prev_score && j > prev_id);
      if (eligible && s >= min_score && after && (s > best || (s == best && j < best_id))) best = s, best_id = j;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      const double os = __shfl_xor(best, off);
      const int oi = __shfl_xor(best_id, off);
      if (os > best || (os == best && oi < best_id)) best = os, best_id = oi;
    }
    if ((threadIdx.x & (kWave - 1)) == 0) s_score[threadIdx.x / kWave] = best, s_id[threadIdx.x / kWave] = best_id;
    __syncthreads();
    best = s_score[0], best_id = s_id[0];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv)
      if (s_score[wv] > best || (s_score[wv] == best && s_id[wv] < best_id)) best = s_score[wv], best_id = s_id[wv];
    __syncthreads();  // (the next round writes s_score again)
    if (best_id == kNone) break;  // (the same in every thread: nothing is left)
    if (threadIdx.x == 0) candidates[(size_t)i * k + round] = best_id, scores[(size_t)i * k + round] = best;
    prev_score = best, prev_id = best_id, ++found;
  }
  for (int t = found + (int)threadIdx.x; t < k; t += kPlaceBlock) candidates[(size_t)i * k + t] = -1, scores[(size_t)i * k + t] = __builtin_nan("");
  if (threadIdx.x == 0) counts[i] = found;
}

hipError_t launch_place_topk(const int *dots, int n_queries, int n, const int *query_ids, const double *r_query, const double *r,
                             int k, double min_score, int exclude_recent, int *candidates, double *scores, int *counts,
                             hipStream_t stream) {
  if (n_queries <= 0) return hipSuccess;
  LaunchGuard guard;
  hipLaunchKernelGGL(k_place_topk, dim3((unsigned)n_queries), dim3(kPlaceBlock), 0, stream, dots, n, query_ids, r_query, r, k, min_score,
                     exclude_recent, candidates, scores, counts);
  return hipGetLastError();
}

}  // namespace dvo_amd
