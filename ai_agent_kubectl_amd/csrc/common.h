// Shared helpers for the CDNA4 (gfx950, MI355X) kernels of the kubectl-agent inference engine.
//
// Conventions (see /opt/skills/guides/cdna_hip_programming.md):
//   * wave = 64 lanes; every block size is a multiple of 64;
//   * bf16 is moved as raw 16-bit words and converted with bit ops (round-to-nearest-even, the
//     same rounding torch uses), loads/stores are 16 B per lane wherever the layout allows
//     (Guideline 13: hipcc never vectorises scalar bf16 accesses);
//   * every launcher is `extern "C"`, takes the HIP stream explicitly and returns the hipError_t
//     of the launch, so the Python side (ops/_hip.py, ctypes) can be captured in hipGraphs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>

typedef uint16_t bf16_t;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

#define KA_DEV __device__ __forceinline__

KA_DEV float bf2f(bf16_t x) { return __uint_as_float(((uint32_t)x) << 16); }

// fp32 -> bf16 round-to-nearest-even (torch's rounding) in one instruction: gfx950's
// v_cvt_pk_bf16_f32 (the bit-twiddling form costs ~6 VALU ops per value, which showed up in the
// VALU-bound softmax / epilogue loops)
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
KA_DEV bf16_t f2bf(float f) { return __builtin_bit_cast(bf16_t, (__bf16)f); }

// two packed bf16 <-> two floats
KA_DEV float lo_f(uint32_t w) { return __uint_as_float(w << 16); }
KA_DEV float hi_f(uint32_t w) { return __uint_as_float(w & 0xffff0000u); }
KA_DEV uint32_t pack2(float a, float b) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2_t{a, b}, bf16x2_t));
}

// Cross-lane exchange within a row of 16 lanes by DPP (a VALU operand modifier: no LDS traffic, unlike
// __shfl_xor, which compiles to ds_bpermute_b32).  Controls (gfx9 DPP): quad_perm [1,0,3,2] = 0xB1,
// quad_perm [2,3,0,1] = 0x4E, row_half_mirror = 0x141, row_mirror = 0x140.
template <int CTRL>
KA_DEV float dpp_f(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

// reduce over the 16 lanes that share (lane >> 4): the column index of an MFMA 16x16 C tile.  Each
// step pairs lanes whose partial results are equal sets of the row, so all 16 lanes end with the
// same (bitwise) value: neighbours, quads, half-rows (mirror within 8), rows (mirror within 16).
KA_DEV float row16_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));
  v = fmaxf(v, dpp_f<0x4E>(v));
  v = fmaxf(v, dpp_f<0x141>(v));
  v = fmaxf(v, dpp_f<0x140>(v));
  return v;
}
KA_DEV float row16_sum(float v) {
  v += dpp_f<0xB1>(v);
  v += dpp_f<0x4E>(v);
  v += dpp_f<0x141>(v);
  v += dpp_f<0x140>(v);
  return v;
}

// whole-wave reduction: the 16-lane row by DPP, then the four rows by two lane swaps
KA_DEV float wave_sum(float v) {
  v = row16_sum(v);
  v += __shfl_xor(v, 16, 64);
  v += __shfl_xor(v, 32, 64);
  return v;
}

KA_DEV f32x4 mfma16x16x32(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

KA_DEV bf16x8 as_bf16x8(const uint4& v) { return __builtin_bit_cast(bf16x8, v); }

#define KA_CHECK_LAUNCH() return (int)hipGetLastError()

// X[m][k] = bf16(silu(GU[m][k]) * GU[m][K + k]) for 8 bf16 lanes — bit-identical to silu_mul_kernel
// (elementwise.hip), so GEMMs that compute the activation while staging their X operand (gemv_ring
// SWIGLU) match the unfused SiLU kernel + GEMM exactly.
KA_DEV u32x4 swiglu8(u32x4 g, u32x4 u) {
  u32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float g0 = lo_f(g[k]), g1 = hi_f(g[k]);
    const float s0 = g0 / (1.f + __expf(-g0)), s1 = g1 / (1.f + __expf(-g1));
    o[k] = pack2(s0 * lo_f(u[k]), s1 * hi_f(u[k]));
  }
  return o;
}

// ---- bf16 dot product -----------------------------------------------------------------------------
// acc + the dot product of two 16-B words of 8 bf16 each, on v_dot2c_f32_bf16: the row-streaming
// GEMVs of gemm_skinny.hip and decode_persistent.hip
KA_DEV float dot8(uint4 w, uint4 x, float acc) {
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.x), __builtin_bit_cast(bf16x2_t, x.x), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.y), __builtin_bit_cast(bf16x2_t, x.y), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.z), __builtin_bit_cast(bf16x2_t, x.z), acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(bf16x2_t, w.w), __builtin_bit_cast(bf16x2_t, x.w), acc, false);
  return acc;
}

// ---- P re-layout scratch of the MFMA attention kernels (attention.hip, decode_persistent.hip) ------
// Per wave: the softmax probabilities leave the MFMA C layout (lane (col, grp) holds rows 4 grp + r,
// keys col and 16 + col) and are re-read in the A layout (lane holds row col, keys 8 grp .. 8 grp + 7).
// 16 rows x PSTR = 40 bf16 (64 B of P + 16 B of padding); 16-B chunk c of row x sits at slot
// c ^ p_slot_xor(x >> 2).  Neighbouring lanes swap one probability so that every lane stores one dword
// (even lanes keys col, col + 1; odd lanes keys 15 + col, 16 + col).  With the 80-B stride and this XOR
// both the stores (2 x 32 lanes on 32 banks) and the ds_read_b128 reads (4 x 16 lanes on 64 banks,
// MI355X_MICROARCH.md §LDS) are conflict-free — found by exhaustive search over strides and XOR maps;
// the previous 64-B rows cost 15-20 % extra LDS cycles.
constexpr int PSTR = 40;
KA_DEV int p_slot_xor(int q) { return (q ^ (q >> 1)) & 1; }
KA_DEV void p_store(bf16_t* pw, int prow, int col, float p0, float p1) {
  const float q0 = dpp_f<0xB1>(p0), q1 = dpp_f<0xB1>(p1);   // lane ^ 1
  const bool even = (col & 1) == 0;
  const int key = even ? col : 15 + col;
  const uint32_t v = even ? pack2(p0, q0) : pack2(q1, p1);
  const int slot = (key >> 3) ^ p_slot_xor(prow >> 2);
  *reinterpret_cast<uint32_t*>(pw + prow * PSTR + (slot << 3) + (key & 7)) = v;
}
KA_DEV bf16x8 p_load(const bf16_t* pw, int col, int grp) {
  return as_bf16x8(*reinterpret_cast<const uint4*>(pw + col * PSTR + ((grp ^ p_slot_xor((col >> 2) & 3)) << 3)));
}

// ---- LDS-DMA GEMM kernels (gemm_big.hip, gemm_mfma.hip) ---------------------------------------------
// compile-time unrolled loop: f(std::integral_constant<int, 0>{}) ... f(..N-1): asm immediates
// ("i" operands) need constants, which a #pragma-unrolled loop variable is not
template <class F, int... S>
KA_DEV void static_for_impl(F&& f, std::integer_sequence<int, S...>) {
  (f(std::integral_constant<int, S>{}), ...);
}
template <int N, class F>
KA_DEV void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}

// wait until at most N of the wave's vector-memory operations (LDS-DMA pieces included) are in flight.
// LDS-DMA pieces do not always complete in issue order, so only N = 0 proves that a piece has landed
// (see the wait schedules in both files).
template <int N>
KA_DEV void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// dispatch index -> logical index, XCD-contiguous (bijective over the grid: consecutive logical
// indices run on one XCD and share its L2)
KA_DEV int xcd_logical(int bid, int nwg) {
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
// logical tile -> (m tile, n tile): GM m-tiles x all n-tiles super-rows
KA_DEV void tile_of(int L, int tiles_m, int tiles_n, int gm, int& tm, int& tn) {
  const int per = gm * tiles_n;
  const int g = L / per, first = g * gm;
  const int rows = min(gm, tiles_m - first);
  const int in = L - g * per;
  tm = first + in % rows;
  tn = in / rows;
}

// ---- host side ------------------------------------------------------------------------------------
// compute units of the current device (256 if the query fails), asked once per source file
static inline int ka_num_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  }
  return n;
}

// Launchers called from another source file: the definer and the caller compile against this line.
// Y[mn] = bf16(sum_k P[k][mn]) (gemm_skinny.hip; gemm_mfma.hip's EPI_P32 path with an output)
extern "C" void ka_splitk_reduce_launch(bf16_t* Y, const float* P, int split, long mn, hipStream_t stream);
// per-slice (max, index) partials -> winner per row (sampling.hip; gemm_big.hip's fused LM head)
extern "C" int ka_argmax_finish(int* out_idx, float* out_val, const float* part_val, const int* part_idx, int rows,
                                int slices, int vocab_offset, hipStream_t stream);
