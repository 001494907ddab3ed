// mpcqp_common.h -- shared device primitives, layouts and the launch record of the batched
// MPC QP solver (included by mpcqp.hip and by the per-horizon solver objects).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/mpcqp.h"

namespace {

constexpr int kWave = 64;
constexpr double kPi = 3.141592653589793;
constexpr double kTwoPi = 6.283185307179586;
constexpr double kMinScaling = 1e-4;
constexpr double kMaxScaling = 1e4;
constexpr double kRhoMin = 1e-6;
constexpr double kRhoMax = 1e6;
constexpr double kDivTol = 1e-30;
constexpr double kRank1Min = 1e-10;  // smallest 1 + delta c'A^{-1}c accepted by a rank-1 update

// ------------------------------------------------------------------ layouts
__host__ __device__ constexpr int model_stride(int N) { return ((11 * N + 10) + 7) / 8 * 8; }

// Solver state per QP (doubles):
//   [0, n*n)            Pbar, symmetric, row-major
//   lane fields         kF* x 64 doubles, lane-contiguous
//   scalars             cscale, admm_ok, admm_it, n_fact
enum LaneField {
  kFq = 0,
  kFD,
  kFx,
  kFE0,
  kFE1,
  kFE2,
  kFlo0,
  kFlo1,
  kFlo2,
  kFhi0,
  kFhi1,
  kFhi2,
  kFw0,
  kFw1,
  kFw2,
  kNumFields
};
__host__ __device__ constexpr int state_lane_off(int N) { return (4 * N * N + 7) / 8 * 8; }
__host__ __device__ constexpr int state_scal_off(int N) { return state_lane_off(N) + kNumFields * kWave; }
__host__ __device__ constexpr int state_stride(int N) { return state_scal_off(N) + 8; }

// ------------------------------------------------------------------ wave primitives (DPP)
template <int CTRL>
__device__ __forceinline__ double dpp(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane(double v, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                          __builtin_amdgcn_readlane(__double2loint(v), l));
}
constexpr int kRowShr1 = 0x111, kRowShr2 = 0x112, kRowShr4 = 0x114, kRowShr8 = 0x118;
constexpr int kRowShl1 = 0x101, kRowShl2 = 0x102, kRowShl4 = 0x104, kRowShl8 = 0x108;
constexpr int kWaveShr1 = 0x138, kWaveShl1 = 0x130;

// DPP with a row mask: rows outside ROWMASK read 0
template <int CTRL, int ROWMASK>
__device__ __forceinline__ double dpp_rows(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, ROWMASK, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, ROWMASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
constexpr int kRowBcast15 = 0x142, kRowBcast31 = 0x143;  // GFX9 wave-level row broadcasts

// inclusive prefix sum over lanes 0..lane: zero-filled row shifts, then the row totals carried
// across rows by row_bcast:15 (rows 1, 3) and row_bcast:31 (rows 2, 3) -- no SGPR round trip
__device__ __forceinline__ double scan_add(double v, int lane) {
  (void)lane;
  v += dpp<kRowShr1>(v);
  v += dpp<kRowShr2>(v);
  v += dpp<kRowShr4>(v);
  v += dpp<kRowShr8>(v);
  v += dpp_rows<kRowBcast15, 0xa>(v);
  v += dpp_rows<kRowBcast31, 0xc>(v);
  return v;
}
// inclusive suffix sum over lanes lane..63
__device__ __forceinline__ double rscan_add(double v, int lane) {
  v += dpp<kRowShl1>(v);
  v += dpp<kRowShl2>(v);
  v += dpp<kRowShl4>(v);
  v += dpp<kRowShl8>(v);
  const double t1 = readlane(v, 16), t2 = readlane(v, 32), t3 = readlane(v, 48);
  const int row = lane >> 4;
  double off = row <= 2 ? t3 : 0.0;
  if (row <= 1) off += t2;
  if (row <= 0) off += t1;
  return v + off;
}
// inclusive prefix / suffix max of non-negative values
__device__ __forceinline__ double scan_max(double v, int lane) {
  v = fmax(v, dpp<kRowShr1>(v));
  v = fmax(v, dpp<kRowShr2>(v));
  v = fmax(v, dpp<kRowShr4>(v));
  v = fmax(v, dpp<kRowShr8>(v));
  const double t0 = readlane(v, 15), t1 = readlane(v, 31), t2 = readlane(v, 47);
  const int row = lane >> 4;
  double off = row >= 1 ? t0 : 0.0;
  if (row >= 2) off = fmax(off, t1);
  if (row >= 3) off = fmax(off, t2);
  return fmax(v, off);
}
__device__ __forceinline__ double rscan_max(double v, int lane) {
  v = fmax(v, dpp<kRowShl1>(v));
  v = fmax(v, dpp<kRowShl2>(v));
  v = fmax(v, dpp<kRowShl4>(v));
  v = fmax(v, dpp<kRowShl8>(v));
  const double t1 = readlane(v, 16), t2 = readlane(v, 32), t3 = readlane(v, 48);
  const int row = lane >> 4;
  double off = row <= 2 ? t3 : 0.0;
  if (row <= 1) off = fmax(off, t2);
  if (row <= 0) off = fmax(off, t1);
  return fmax(v, off);
}
// max / min without LLVM's IEEE-mode operand canonicalization (it adds a v_max_f64 x, x, x for
// every operand not known to be canonical -- DPP results, values kept opaque across solver
// iterations).  No kernel here produces signalling NaNs, and on quiet operands the instruction
// is IEEE maxNum / minNum, i.e. fmax / fmin bit for bit.
__device__ __forceinline__ double max_nc(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double min_nc(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// wave-uniform sum / max: the inclusive scan's last lane
__device__ __forceinline__ double wave_sum(double v) { return readlane(scan_add(v, 0), 63); }
// two wave sums at once, each with scan_add's association: the steps alternate, so one sum's DPP moves
// and their wait states issue under the other's add
__device__ __forceinline__ void wave_sum2(double& a, double& b) {
  a += dpp<kRowShr1>(a);
  b += dpp<kRowShr1>(b);
  a += dpp<kRowShr2>(a);
  b += dpp<kRowShr2>(b);
  a += dpp<kRowShr4>(a);
  b += dpp<kRowShr4>(b);
  a += dpp<kRowShr8>(a);
  b += dpp<kRowShr8>(b);
  a += dpp_rows<kRowBcast15, 0xa>(a);
  b += dpp_rows<kRowBcast15, 0xa>(b);
  a += dpp_rows<kRowBcast31, 0xc>(a);
  b += dpp_rows<kRowBcast31, 0xc>(b);
  a = readlane(a, 63);
  b = readlane(b, 63);
}
__device__ __forceinline__ double wave_max(double v) {  // v >= 0
  v = max_nc(v, dpp<kRowShr1>(v));
  v = max_nc(v, dpp<kRowShr2>(v));
  v = max_nc(v, dpp<kRowShr4>(v));
  v = max_nc(v, dpp<kRowShr8>(v));
  v = max_nc(v, dpp_rows<kRowBcast15, 0xa>(v));
  v = max_nc(v, dpp_rows<kRowBcast31, 0xc>(v));
  return readlane(v, 63);
}
// one step of four max reductions at once (values >= 0, or quiet NaNs, which v_max_f64 drops against a
// number as fmax does): the four moves, then the four maxima, so each reduction's DPP moves and their
// wait states issue under the other three's
#define MPCQP_MAX4_STEP(MOVE)                                             \
  {                                                                       \
    const double ta = MOVE(a), tb = MOVE(b), tc = MOVE(c), td = MOVE(d); \
    a = max_nc(a, ta);                                                    \
    b = max_nc(b, tb);                                                    \
    c = max_nc(c, tc);                                                    \
    d = max_nc(d, td);                                                    \
  }
// the steps of wave_max within the 16-lane rows and from row 0 / 2 into row 1 / 3: lanes 31 and 63 hold
// the maxima of their 32-lane halves
__device__ __forceinline__ void half_max4_steps(double& a, double& b, double& c, double& d) {
  MPCQP_MAX4_STEP(dpp<kRowShr1>)
  MPCQP_MAX4_STEP(dpp<kRowShr2>)
  MPCQP_MAX4_STEP(dpp<kRowShr4>)
  MPCQP_MAX4_STEP(dpp<kRowShr8>)
  MPCQP_MAX4_STEP((dpp_rows<kRowBcast15, 0xa>))
}
// four wave maxima at once (max is exact and order-free: each is wave_max's value)
__device__ __forceinline__ void wave_max4(double& a, double& b, double& c, double& d) {
  half_max4_steps(a, b, c, d);
  MPCQP_MAX4_STEP((dpp_rows<kRowBcast31, 0xc>))
  a = readlane(a, 63);
  b = readlane(b, 63);
  c = readlane(c, 63);
  d = readlane(d, 63);
}
#undef MPCQP_MAX4_STEP
// lane i <- lane i-2 (0 for i < 2);  lane i <- lane i+2 (0 past the wave)
__device__ __forceinline__ double shr2(double v) { return dpp<kWaveShr1>(dpp<kWaveShr1>(v)); }
__device__ __forceinline__ double shl2(double v) { return dpp<kWaveShl1>(dpp<kWaveShl1>(v)); }
__device__ __forceinline__ double shr4(double v) { return shr2(shr2(v)); }
__device__ __forceinline__ double shl4(double v) { return shl2(shl2(v)); }
__device__ __forceinline__ bool wave_any(bool b) { return __ballot(b) != 0ull; }

// ---- register broadcasts for the dense row-per-lane products (no LDS)
// A dense product over a vector v distributed one element per lane needs every lane to see
// every v_j.  bcast() replicates each 16-lane row of v into all four rows with the gfx950
// permlane swaps (w[c] lane l = v[16c + (l & 15)]); v_fmac_f64 with DPP row_newbcast:L then
// reads lane L of each row's copy as its multiplicand, so a broadcast-FMA is ONE VALU
// instruction with no memory latency.  Must run with all 64 lanes active.
template <int NW>  // rows needed: ceil(n / 16)
__device__ __forceinline__ void bcast(double v, double w[4]) {
  const int lo = __double2loint(v), hi = __double2hiint(v);
  const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);  // rows {0,0,2,2} / {1,1,3,3}
  const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  const auto la = __builtin_amdgcn_permlane32_swap(l16[0], l16[0], false, false);  // row 0 x4 / row 2 x4
  const auto ha = __builtin_amdgcn_permlane32_swap(h16[0], h16[0], false, false);
  w[0] = __hiloint2double(ha[0], la[0]);
  if constexpr (NW > 1) {
    const auto lb = __builtin_amdgcn_permlane32_swap(l16[1], l16[1], false, false);  // row 1 x4 / row 3 x4
    const auto hb = __builtin_amdgcn_permlane32_swap(h16[1], h16[1], false, false);
    w[1] = __hiloint2double(hb[0], lb[0]);
    if constexpr (NW > 3) w[3] = __hiloint2double(hb[1], lb[1]);
  }
  if constexpr (NW > 2) w[2] = __hiloint2double(ha[1], la[1]);
  // DPP reads of a VGPR need two wait states after its VALU write; tie the pad to w
  if constexpr (NW == 1) asm volatile("s_nop 1" : "+v"(w[0]));
  if constexpr (NW == 2) asm volatile("s_nop 1" : "+v"(w[0]), "+v"(w[1]));
  if constexpr (NW == 3) asm volatile("s_nop 1" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]));
  if constexpr (NW == 4) asm volatile("s_nop 1" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]));
}
// The same for a vector that lives in the lanes of rows 0-1 of each half (n <= 32 in the whole-wave
// layout, n <= 30 in a half): one permlane16 swap per word puts row 0 / row 1 of each half into both
// of its rows (w[0] / w[1]); with n <= 16 (NW = 1) row 0 is already where its lanes read it, and no
// lane moves at all (whole-wave layout only).  The lanes of the other rows read their own rows'
// values there: padding, which the callers keep finite (exact zeros).
template <int NW>
__device__ __forceinline__ void bcast_rows01(double v, double w[4]) {
  static_assert(NW <= 2, "two 16-lane rows");
  if constexpr (NW == 1) {
    w[0] = v;
    asm volatile("s_nop 1" : "+v"(w[0]));
  } else {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    const auto l16 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);  // rows {0,0,2,2} / {1,1,3,3}
    const auto h16 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    w[0] = __hiloint2double(h16[0], l16[0]);
    w[1] = __hiloint2double(h16[1], l16[1]);
    // DPP reads of a VGPR need two wait states after its VALU write; tie the pad to w
    asm volatile("s_nop 1" : "+v"(w[0]), "+v"(w[1]));
  }
}
// acc += w[lane 16*row + L] * m   (one v_fmac_f64_dpp)
template <int L>
__device__ __forceinline__ void fmac_bc(double& acc, double w, double m) {
  asm("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(w), "v"(m), "i"(L));
}
// ---- the sweep's pivot step (Ctx::sweep, Ctx::sweep_reg)
// One step's coefficient and new r[k] from rk = r[k] and inv = 1/d, five VALU instructions:
//   every lane:        coef = -(rk * inv)  (the product with inv's source negation: a product's sign
//                      is the xor of its operands' signs, so these are the negated product's bits,
//                      zeros and infinities included)  and  rk = rk * inv;
//   the pivot lanes:   coef = inv - 1.0  and  rk = -inv  (inv * -1.0: exact, no rounding, and inv, an
//                      FMA's result, is already in the kernel's denormal mode), written under an exec
//                      mask of those lanes alone.
// K2 == K, a QP on the whole wave: lane K, and all 64 lanes active afterwards -- as they are before: the
// whole-wave sweep's permlane and DPP broadcasts read every lane.  Otherwise the pair layout: lanes K and
// K2, cut to the active lanes (the other half may be masked off) and the exec mask restored.  The mask is
// built from inline constants inside the statement (in exec itself, or in vcc): as an SGPR operand the
// compiler keeps the sweep's 2N masks live through the kernel and spills SGPRs, and the fused loops
// have none to spare.  One asm statement, so the compiler
// neither pads between its instructions nor rewrites -(rk * inv) into integer operations on rk * inv.
template <int K, int K2>
__device__ __forceinline__ void pivot_step(double& coef, double& rk, double inv) {
  if constexpr (K2 == K) {  // the whole wave is active: its sweep's broadcasts need that already
    asm volatile(
        "v_mul_f64 %[c], %[r], -%[i]\n\t"
        "v_mul_f64 %[r], %[r], %[i]\n\t"
        "s_lshl_b64 exec, 1, %[k]\n\t"
        "v_add_f64 %[c], %[i], -1.0\n\t"
        "v_mul_f64 %[r], %[i], -1.0\n\t"
        "s_mov_b64 exec, -1"
        : [c] "=&v"(coef), [r] "+v"(rk)
        : [i] "v"(inv), [k] "n"(K)
        : "scc");
  } else {
    uint64_t saved;
    asm volatile(
        "s_lshl_b64 vcc, 1, %[k]\n\t"
        "v_mul_f64 %[c], %[r], -%[i]\n\t"
        "s_bitset1_b64 vcc, %[k2]\n\t"
        "v_mul_f64 %[r], %[r], %[i]\n\t"
        "s_and_saveexec_b64 %[sv], vcc\n\t"
        "v_add_f64 %[c], %[i], -1.0\n\t"
        "v_mul_f64 %[r], %[i], -1.0\n\t"
        "s_mov_b64 exec, %[sv]"
        : [c] "=&v"(coef), [r] "+v"(rk), [sv] "=&s"(saved)
        : [i] "v"(inv), [k] "n"(K), [k2] "n"(K2)
        : "scc", "vcc");
  }
}

// ---- lane policies of the one-wave solver: a QP owns the whole wave (Lanes<false>, the layout
// above) or one 32-lane half of it (Lanes<true>: two QPs per wave, lanes 0-31 and 32-63, for
// n = 2N <= 30, where a whole-wave QP leaves lanes 30..63 computing on padding).  Every cross-lane
// operation of a half stays inside it: 16-lane-row DPP, permlane16 swaps (rows 0<->1, 2<->3),
// row_bcast:15 into rows 1 / 3, ds_bpermute within 32 lanes -- so the two QPs of a wave may take
// different branches (the other half is masked off), and a half's sums and scans add the same
// values in the same order as the whole-wave ones (lanes past n hold zeros in both layouts).
template <bool Pair>
struct Lanes;

template <>
struct Lanes<false> {
  static constexpr int kLanes = kWave;
  template <int NW>
  __device__ __forceinline__ static void vbcast(double v, double w[4]) {
    if constexpr (NW <= 2)
      bcast_rows01<NW>(v, w);  // rows 2-3 are padding: no permlane32 stage
    else
      bcast<NW>(v, w);
  }
  template <int K>
  __device__ __forceinline__ static double read(double v) { return readlane(v, K); }
  __device__ __forceinline__ static double readv(double v, int l) { return readlane(v, l); }
  __device__ __forceinline__ static int uniform(int l) { return __builtin_amdgcn_readfirstlane(l); }
  __device__ __forceinline__ static double sum(double v) { return wave_sum(v); }
  __device__ __forceinline__ static void sum2(double& a, double& b) { wave_sum2(a, b); }
  __device__ __forceinline__ static double max(double v) { return wave_max(v); }
  __device__ __forceinline__ static void max4(double& a, double& b, double& c, double& d) { wave_max4(a, b, c, d); }
  __device__ __forceinline__ static bool any(bool b) { return wave_any(b); }
  __device__ __forceinline__ static uint64_t ballot(bool b) { return __ballot(b); }
  __device__ __forceinline__ static double shr2(double v) { return ::shr2(v); }
  __device__ __forceinline__ static double shl2(double v) { return ::shl2(v); }
  __device__ __forceinline__ static double shr4(double v) { return ::shr4(v); }
  __device__ __forceinline__ static double shl4(double v) { return ::shl4(v); }
  __device__ __forceinline__ static double shr1(double v) { return dpp<kWaveShr1>(v); }  // lane 0 <- 0
  __device__ __forceinline__ static double shl1(double v) { return dpp<kWaveShl1>(v); }  // lane 63 <- 0
  __device__ __forceinline__ static double scan(double v, int lane) { return scan_add(v, lane); }
  __device__ __forceinline__ static double shfl(double v, int src) { return __shfl(v, src, kWave); }
};

// lane L of each 16-lane row, to the whole row (one v_mov_b32_dpp row_newbcast per word)
template <int L>
__device__ __forceinline__ double row_bc(double v) {
  const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x150 + L, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x150 + L, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// Every result that crosses lanes is pinned (an empty asm volatile) where it is computed: the
// compiler turns a lane-dependent select of a DPP result (the half-boundary cuts below) into a
// branch and sinks the DPP into it, where its source lanes are masked off and read as 0.
template <>
struct Lanes<true> {
  static constexpr int kLanes = 32;
  __device__ __forceinline__ static int hl() { return (int)threadIdx.x & 31; }  // lane within the half
  __device__ __forceinline__ static double pin(double v) {
    asm volatile("" : "+v"(v));
    return v;
  }
  // w[c] lane l = v[16c + (l & 15)] of l's own half (c = 0, 1): one permlane16 swap per word, also
  // at NW = 1 (the sweep reads its pivot from w in every lane of the half)
  template <int NW>
  __device__ __forceinline__ static void vbcast(double v, double w[4]) {
    static_assert(NW <= 2, "a half holds 32 lanes");
    bcast_rows01<2>(v, w);
  }
  template <int K>
  __device__ __forceinline__ static double read(double v) {
    double w[4];
    bcast_rows01<2>(v, w);
    return pin(row_bc<K % 16>(w[K / 16]));
  }
  __device__ __forceinline__ static double readv(double v, int l) { return pin(__shfl(v, l, 32)); }
  __device__ __forceinline__ static int uniform(int l) { return l; }
  // inclusive scan within the rows, then rows 1 / 3 take rows 0 / 2's total: lane 31 / 63 = the sum
  __device__ __forceinline__ static double scan(double v, int lane) {
    (void)lane;
    v += dpp<kRowShr1>(v);
    v += dpp<kRowShr2>(v);
    v += dpp<kRowShr4>(v);
    v += dpp<kRowShr8>(v);
    v += dpp_rows<kRowBcast15, 0xa>(v);
    return pin(v);
  }
  __device__ __forceinline__ static double sum(double v) { return read<31>(scan(v, 0)); }
  __device__ __forceinline__ static void sum2(double& a, double& b) {
    a = sum(a);
    b = sum(b);
  }
  __device__ __forceinline__ static double max(double v) {  // v >= 0
    v = max_nc(v, dpp<kRowShr1>(v));
    v = max_nc(v, dpp<kRowShr2>(v));
    v = max_nc(v, dpp<kRowShr4>(v));
    v = max_nc(v, dpp<kRowShr8>(v));
    v = max_nc(v, dpp_rows<kRowBcast15, 0xa>(v));
    return read<31>(v);
  }
  __device__ __forceinline__ static void max4(double& a, double& b, double& c, double& d) {  // >= 0 or quiet NaN
    half_max4_steps(a, b, c, d);
    a = read<31>(a);
    b = read<31>(b);
    c = read<31>(c);
    d = read<31>(d);
  }
  __device__ __forceinline__ static uint64_t ballot(bool b) {
    const uint64_t m = __ballot(b);
    return (threadIdx.x & 32) ? (m >> 32) : (m & 0xffffffffull);
  }
  __device__ __forceinline__ static bool any(bool b) { return ballot(b) != 0ull; }
  // wave shifts, cut at the half boundary (what crosses it reads as 0, as past the wave's ends)
  __device__ __forceinline__ static double shr2(double v) {
    const double d = pin(::shr2(v));
    return hl() >= 2 ? d : 0.0;
  }
  __device__ __forceinline__ static double shl2(double v) {
    const double d = pin(::shl2(v));
    return hl() < 30 ? d : 0.0;
  }
  __device__ __forceinline__ static double shr4(double v) { return shr2(shr2(v)); }
  __device__ __forceinline__ static double shl4(double v) { return shl2(shl2(v)); }
  __device__ __forceinline__ static double shr1(double v) {
    const double d = pin(dpp<kWaveShr1>(v));
    return hl() >= 1 ? d : 0.0;
  }
  __device__ __forceinline__ static double shl1(double v) {
    const double d = pin(dpp<kWaveShl1>(v));
    return hl() < 31 ? d : 0.0;
  }
  __device__ __forceinline__ static double shfl(double v, int src) { return pin(__shfl(v, src, 32)); }
};

// compile-time loop: f(std::integral_constant<int, I>) for I in [B, E)
template <int B, int E>
struct Unroll {
  template <class F>
  __device__ __forceinline__ static void run(F&& f) {
    if constexpr (B < E) {
      f(std::integral_constant<int, B>{});
      Unroll<B + 1, E>::run(f);
    }
  }
};

// Every kernel runs one wavefront per workgroup, and the LDS operations of one wavefront
// execute in program order: a broadcast through LDS needs only a compiler-level ordering
// point (wavefront-scope fence), not an s_barrier with its lgkmcnt(0) drain.
__device__ __forceinline__ void lds_sync() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// ------------------------------------------------------------------ phase marks
// Built only with -DMPCQP_PHASE_MARKS for static analysis of the device assembly (never in the measured
// library): an assembly comment where a solver phase begins, so tools/isa_breakdown.py can attribute
// every instruction of k_solve<N> to the phase it executes in and weight it by the phase's count.
#ifdef MPCQP_PHASE_MARKS
#define MPCQP_MARK(name) asm volatile(";@phase " name)
#else
#define MPCQP_MARK(name)
#endif

// ------------------------------------------------------------------ diagnostic stamps
// Built only with -DMPCQP_STAMPS (never in the measured library): per-phase s_memtime
// cycle sums, flushed once per wave into g_stamps[] (read by mpcqp_debug_stamps).
#ifdef MPCQP_STAMPS
__device__ unsigned long long g_stamps[32];
struct Stamps {
  unsigned long long acc[6] = {0, 0, 0, 0, 0, 0};
  unsigned long long t = 0;
  __device__ __forceinline__ void begin() {
    __builtin_amdgcn_sched_barrier(0);
    t = __builtin_amdgcn_s_memtime();
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void end(int s) {
    __builtin_amdgcn_sched_barrier(0);
    acc[s] += __builtin_amdgcn_s_memtime() - t;
    __builtin_amdgcn_sched_barrier(0);
  }
  __device__ __forceinline__ void flush(int base) {
    if (threadIdx.x == 0)
      for (int s = 0; s < 6; ++s) atomicAdd(&g_stamps[base + s], acc[s]);
  }
};
#else
struct Stamps {
  __device__ __forceinline__ void begin() {}
  __device__ __forceinline__ void end(int) {}
  __device__ __forceinline__ void flush(int) {}
};
#endif

__device__ __forceinline__ double limit_scaling(double v) {
  return v < kMinScaling ? 1.0 : (v > kMaxScaling ? kMaxScaling : v);
}

// numpy float mod (npy_divmod) for b > 0
__device__ __forceinline__ double np_mod(double a, double b) {
  double m = fmod(a, b);
  if (m != 0.0) {
    if (m < 0.0) m += b;
  } else {
    m = 0.0;
  }
  return m;
}

// Per-QP parameter classes (mpcqp_build_mixed): QP b's block is P[cls[b]] of a K-entry table.  The
// index is checked before it indexes anything: false for (unsigned)c >= K, and thread 0 has then
// written status[b] = MPCQP_BAD_CLASS and zero iters (nothing else of the QP is written).  The caller
// returns at once, before any barrier; c is uniform over the QP's wave / workgroup.
__device__ __forceinline__ bool class_ok(int c, int K, int b, int32_t* __restrict__ statuso,
                                         int32_t* __restrict__ iterso) {
  if ((unsigned)c < (unsigned)K) return true;
  if (threadIdx.x == 0) {
    statuso[b] = MPCQP_BAD_CLASS;
    if (iterso)
      for (int i = 0; i < 4; ++i) iterso[4 * (size_t)b + i] = 0;
  }
  return false;
}

// ------------------------------------------------------------------ the ADMM / polish schedule
// The ADMM loop state of one QP (admm_run in mpcqp_solve.h, mid_admm in mpcqp_mid.hip).  It lives in the
// family's driver: the ADMM function stops at a termination check that asks for an early polish and the
// driver resumes it after a failed attempt, so a kernel holds ONE inlined copy of the polish (attempts,
// final polish and method newton share the driver's call site) -- the polish is a third of the one-wave
// kernel's code, which is larger than the 64 KB instruction cache.
struct AdmmState {
  double x, z[3], y[3], rho;
  double rho_next;  // the adaptive-rho update of the check that stopped for an attempt
  int it, nfact;
  bool need_fact;   // form + sweep at the next entry (start, rho change, after a failed attempt)
  bool rho_change;  // rho_next is pending (applied after a failed attempt)
};
// What the ADMM function stops for: kAdmmBad (numerical error), kAdmmConverged (eps_abs / eps_rel met),
// kAdmmAttempt (a check asks for an early polish; rho_change / rho_next hold that check's adaptive-rho
// decision), kAdmmApprox / kAdmmMaxIter (max_iter reached within / outside 10x the tolerances: OSQP's
// solved_inaccurate / max_iter_reached).
enum : int { kAdmmBad = -1, kAdmmMaxIter = 0, kAdmmConverged = 1, kAdmmApprox = 3, kAdmmAttempt = 4 };

}  // namespace

namespace mpcqp {
// One solve launch (device pointers; outputs may be null).
struct Launch {
  const mpcqp_params* p;
  int B;
  const double* model;
  double* state;
  double *u0, *X, *U;
  int32_t *st, *it;
  uint8_t* ac;
  const uint8_t* mask;  // QP b is solved iff mask == nullptr or mask[b] != 0 (fleet steps)
  // K1 fused into the solve: with ref != nullptr the kernel builds each QP's LTV model from the
  // caller's inputs itself (one-wave kernel); otherwise it reads `model` (K1 / fleet output)
  const double* x0 = nullptr;
  const double* ref = nullptr;
  const double* u_prev = nullptr;
  // per-QP parameter classes (mpcqp_build_mixed): with cls != nullptr QP b runs under table[cls[b]]
  // (K blocks in device memory, the workspace's horizon and kernel family) and p only selects the kernel
  const mpcqp_params* table = nullptr;
  const int32_t* cls = nullptr;
  int K = 0;
  // mpcqp_set_class_pairing: the slot table of k_class_slots over this batch (2 x mpcqp_class_slot_waves(B, K)
  // entries), two QPs of one class per wave (k_solve_pair_mixed)
  const int32_t* slots = nullptr;
  // a caller's guess (mpcqp_solve_warm): B x 2 x N in the layout of U, and the attempt's pass limit
  const double* guess = nullptr;
  int guess_passes = 0;
};

typedef void (*launcher_t)(hipStream_t, const Launch&);
constexpr int kPairMaxHorizon = 15;  // n = 2N <= 30: two QPs per wave
// mpcqp_class_slot_waves: the grid of a class-paired mixed launch, (V + min(K + 1, V)) / 2 -- at least
// the used waves (V + odd buckets) / 2 of the K + 1 buckets, at most V
inline int class_slot_waves(int V, int K) {
  if (V <= 0 || K < 0) return 0;
  const long long buckets = (long long)K + 1;
  return (int)(((long long)V + (buckets < V ? buckets : (long long)V)) / 2);
}
// The config-5 replan trigger inside the fused loop (mpcqp_swarm_loop): after each step a RUNNING
// vehicle farther than replan_distance from ref[path_idx], or an ABORTED one, with replans left leaves
// the loop as MPCQP_FLEET_REPLAN_* with its replanning problem in start_goal.  max_replans = 0: off.
struct LoopTrigger {
  double replan_distance;
  int max_replans;
  const int32_t* replans;
  double* start_goal;
  // workgroup -> vehicle (nullptr: identity).  The fused loops dispatch the vehicles longest
  // reference first: a vehicle's step count follows its reference length, and the slowest
  // vehicles started last would set the run's tail once the vehicles outnumber the wave slots.
  const int32_t* order = nullptr;
  bool pair = false;  // two vehicles per wave (N <= 15): k_fleet_loop<N, true>
};
// The B = 1 server (mpcqp_solve_served): one resident wave that solves the QP of the workspace's
// staging block each time the host raises `req`, then publishes `done`.  In pinned, mapped,
// coherent host memory; req and done on separate 64-byte lines.
struct ServeBox {
  uint32_t req;
  uint32_t pad0[15];
  uint32_t done;
  uint32_t pad1[15];
};
constexpr uint32_t kServeStop = 0xffffffffu;  // req value that ends the server
struct ServeLaunch {
  ServeBox* box;      // device address of the mailbox
  const double* in;   // device address of the staging input block (x0 | ref | u_prev)
  uint8_t* out;       // device address of the staging output block
  int32_t off[6];     // output block offsets (u0, X, U, status, iters, active)
  uint64_t idle_ticks;  // s_memrealtime ticks (100 MHz) without a request after which the wave exits
};
typedef void (*serve_t)(hipStream_t, const mpcqp_params&, const ServeLaunch&);
// The server from a caller's guess (mpcqp_solve_served_warm, k_serve_warm): k_serve's launch plus the
// workspace's guess block (mpcqp_stage_guess): 2 x N doubles in the layout of U, and behind them the
// request's guess_passes.  The host writes both before it raises box->req.
struct ServeWarmLaunch {
  ServeLaunch serve;
  const double* guess;    // device address of the guess block
  const int32_t* passes;  // device address of guess_passes (the block's last 8 bytes)
};
typedef void (*serve_warm_t)(hipStream_t, const mpcqp_params&, const ServeWarmLaunch&);
// The changing map of mpcqp_swarm_loop_map (k_swarm_loop_map): the grids by epoch and the blocked test's
// lookahead, with the grid size of the swarm's planner.  Not part of LoopTrigger: that struct is a by-value
// argument of every loop kernel, and a field more would move all of their kernel-argument offsets.
struct LoopMap {
  const uint8_t* grids = nullptr;  // T x height x width, 1 = free
  int num_grids = 0, epoch_steps = 1, lookahead = 0;
  int width = 0, height = 0;
  int32_t* grid_of = nullptr;      // V: the grid of the vehicle's last trigger
  uint8_t* cause = nullptr;        // V x max_replans (nullable): MPCQP_REPLAN_*
};
// One fused-loop launch (device pointers), the loops' counterpart of Launch: k_fleet_loop (tr.pair: two
// vehicles per wave), k_fleet_loop_mixed (cls != nullptr), k_fleet_loop_warm, k_swarm_loop_warm and k_swarm_loop_map
// (map) read what they need of it.
struct LoopLaunch {
  const mpcqp_params* P;  // {nominal, relaxed}; with cls the 2 K interleaved blocks {nominal[c], relaxed[c]}
  const mpcqp_fleet* f;
  int steps;
  // live in k_fleet_loop, k_swarm_loop_warm and k_swarm_loop_mixed[_warm] (the swarm's calls); the mixed and
  // warm fleet loops read only its dispatch order, and the carry loop its pairing too
  LoopTrigger tr;
  const int32_t* cls = nullptr;  // a class per vehicle (V indices) into the K classes
  int K = 0;
  // mpcqp_set_class_pairing (with cls): the workspace's slot table, set by the caller and filled on the
  // stream by enqueue_fused_loop; two vehicles of one class per wave (k_fleet_loop_pair_mixed)
  int32_t* slots = nullptr;
  int guess_passes = 0;  // the warm loop's pass limit per attempt
  double* carry = nullptr;  // k_fleet_loop_warm_carry: the carried guess, V x 2 x N (nullable)
  LoopMap map;  // k_swarm_loop_map only
};
typedef void (*fleet_loop_t)(hipStream_t, const LoopLaunch&);
// The kernels of one horizon of the one-wave family (N < MPCQP_WIDE_MIN_HORIZON; the launch_*<N>
// templates of mpcqp_solve.h), one member per launcher.  The object that instantiates a horizon registers
// it from a namespace-scope initialiser (register_horizons, mpcqp_solve.h: member by member, since many
// share one type); an all-null entry is a horizon not compiled in.
struct HorizonKernels {
  launcher_t solve;               // k_solve
  launcher_t mixed;               // k_solve_mixed: a parameter block per QP
  launcher_t pair;                // k_solve_pair: two QPs per wave, fused K1; nullptr above kPairMaxHorizon
  serve_t serve;                  // k_serve: the B = 1 server
  fleet_loop_t loop;              // k_fleet_loop: the fused closed loop; two vehicles per wave where tr.pair
  fleet_loop_t loop_mixed;        // k_fleet_loop_mixed: a class per vehicle; k_fleet_loop_pair_mixed where L.slots
  launcher_t warm;                // k_solve_warm: from a caller's guess
  fleet_loop_t loop_warm;         // k_fleet_loop_warm: the fused loop, each step from the one before
  serve_warm_t serve_warm;        // k_serve_warm: the B = 1 server from a caller's guess
  launcher_t pair_warm;           // k_solve_pair_warm: two QPs per wave from a guess; nullptr above kPairMaxHorizon
  fleet_loop_t loop_warm_carry;   // k_fleet_loop_warm_carry: the guess carried across launches; tr.pair as loop
  fleet_loop_t swarm_warm;        // k_swarm_loop_warm: the warm loop with the live replan trigger; tr.pair as loop
  fleet_loop_t swarm_mixed;       // k_swarm_loop_mixed: the swarm's cold loop, a class per vehicle; never paired
  fleet_loop_t swarm_mixed_warm;  // k_swarm_loop_mixed_warm: its warm loop; never paired
  launcher_t pair_mixed;          // k_solve_pair_mixed: two QPs of one class per wave; nullptr above kPairMaxHorizon
  fleet_loop_t swarm_map;         // k_swarm_loop_map: the swarm's cold loop on a changing map (L.map); never paired
};
// fills entry N of the table in mpcqp.hip (constant-initialised, so the order of the objects'
// initialisers does not matter)
void register_horizon(int N, const HorizonKernels& k);
// The one read of that table: the one-wave kernels of the parameter block's horizon; nullptr when it
// runs another kernel family (long horizons, reproducible mode) or, for the entry points that keep no
// debug state, with debug_state.  A caller takes the member it needs and tests it for null (a horizon
// not compiled in).  Defined in mpcqp.hip.
const HorizonKernels* one_wave(const mpcqp_params& p, bool debug_ok = false);
// k_solve_pair / k_fleet_loop<N, true> for `count` QPs or vehicles of this workspace's launch?
bool use_pairs(const mpcqp_ws* ws, int count);
// k_solve_pair_mixed / k_fleet_loop_pair_mixed for a mixed launch of this workspace (its class table)?
// Under mpcqp_set_class_pairing, where the paired kernels exist (N <= 15, fast mode, no debug_state) and
// the table has at most MPCQP_CLASS_SLOT_MAX_CLASSES classes.  Defined in mpcqp.hip.
bool use_class_pairs(const mpcqp_ws* ws);
// mpcqp_class_slots after its argument checks (mpcqp_fleet.hip): the slot kernel on the stream
void enqueue_class_slots(int V, int K, const int32_t* cls, const int32_t* seq, int32_t* slots, hipStream_t s);
// the long-horizon solve (N >= MPCQP_WIDE_MIN_HORIZON; mpcqp_wide.hip): one 256-thread workgroup
// per QP, L.state = its workspace (wide_stride(N) doubles per QP)
void launch_solve_wide(hipStream_t s, const Launch& L);
// the same with a parameter block per QP (k_solve_wide_mixed; an object of its own)
void launch_solve_wide_mixed(hipStream_t s, const Launch& L);
size_t wide_stride(int horizon);
// the mid-horizon fast solve (MPCQP_WIDE_MIN_HORIZON <= N <= MPCQP_MID_MAX_HORIZON, mpcqp_mid.hip):
// one workgroup of 4 x (1 or 2) waves per QP, instantiated per padded horizon bucket NT; L.state = its
// workspace (mid_stride(N) doubles per QP: the scaled Hessian)
template <int NT>
void launch_solve_mid(hipStream_t s, const Launch& L);
// the same with a parameter block per QP (k_solve_mid_mixed<NT>; an object of its own per bucket)
template <int NT>
void launch_solve_mid_mixed(hipStream_t s, const Launch& L);
inline int mid_bucket(int N) { return N <= 40 ? 40 : (N <= 48 ? 48 : (N <= 56 ? 56 : 64)); }  // N >= 33
inline size_t mid_stride(int N) { return (size_t)2 * mid_bucket(N) * 128; }
// the solve of this parameter block runs a workgroup-per-QP kernel (long horizon or reproducible)
bool wide_solve(const mpcqp_params& p);
// launcher of the parameter block's horizon / kernel (nullptr when not compiled in); defined in mpcqp.hip
launcher_t launcher(const mpcqp_params& p);
// records msg as mpcqp_last_error() of the calling thread and returns code; defined in mpcqp.hip
int fail(int code, const std::string& msg);
// after a kernel launch: MPCQP_OK, or MPCQP_E_HIP with "<what> launch: <HIP's error>"
inline int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(MPCQP_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
  return MPCQP_OK;
}
// Makes `device` current for a scope and restores the caller's device on exit (only when one was
// read and differs).  err: the first failure of the two calls.
struct DeviceGuard {
  int device, cur = -1;
  hipError_t err;
  explicit DeviceGuard(int dev) : device(dev) {
    err = hipGetDevice(&cur);
    if (err == hipSuccess && cur != device) err = hipSetDevice(device);
  }
  ~DeviceGuard() {
    if (cur >= 0 && cur != device) (void)hipSetDevice(cur);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
// `count` T of pinned host memory that the device reads and writes in place (mapped, coherent): the
// blocks of the B = 1 path.  alloc() runs on the current device and zeroes the block; on failure
// nothing is held.
template <class T>
struct Mapped {
  T* host = nullptr;
  T* dev = nullptr;  // the same block's device address
  hipError_t alloc(size_t count) {
    void *h = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&h, sizeof(T) * count, hipHostMallocMapped | hipHostMallocCoherent);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&d, h, 0);
    if (e != hipSuccess) {
      if (h) (void)hipHostFree(h);
      return e;
    }
    std::memset(h, 0, sizeof(T) * count);
    host = static_cast<T*>(h);
    dev = static_cast<T*>(d);
    return hipSuccess;
  }
  void release() {
    if (host) (void)hipHostFree(host);
    host = dev = nullptr;
  }
};
}  // namespace mpcqp

// Workspace of one device: parameter block + per-QP model (K1 output) and solver state.
struct mpcqp_ws {
  mpcqp_params p;
  int max_batch = 0;
  int device = 0;
  // What the workspace holds for mpcqp_solve: the batch of the last successful mpcqp_build /
  // mpcqp_build_mixed; its inputs when the model is built inside the solve (fused K1, else null); its
  // class indices when it was a mixed build (else null).  New parameters, a new class table and every
  // fleet or swarm call that uses the workspace invalidate it.  built() and invalidate() are the only
  // writers.
  struct Build {
    bool valid = false;
    int B = 0;
    const double *x0 = nullptr, *ref = nullptr, *u_prev = nullptr;
    const int32_t* cls = nullptr;
  };
  Build build;
  void invalidate() { build = Build{}; }
  void built(int B, const double* x0, const double* ref, const double* u_prev, const int32_t* cls) {
    build = Build{true, B, x0, ref, u_prev, cls};
  }
  // per-QP model (K1 output) and solver state, allocated by ensure_buffers at the first call that
  // needs them: the fused one-wave solve builds the model on chip and keeps the scaled problem
  // there, so a workspace that only runs it holds neither (22 KB per QP at N = 20)
  double* model = nullptr;
  double* state = nullptr;
  // device copies of the parameter blocks of the last mpcqp_fleet_loop (nominal, relaxed): the fused
  // loop selects its block per solve, which a kernel argument cannot be (the compiler copies a
  // run-time-selected argument block to scratch); written by a kernel on the launch stream
  mpcqp_params* dparams = nullptr;
  // the fused loop's dispatch order (max_batch vehicles), written by k_fleet_order on the stream
  int32_t* dorder = nullptr;
  // the B = 1 path (mpcqp_stage / mpcqp_solve_staged): mapped host blocks and a private stream
  mpcqp::Mapped<double> stage_in;    // x0 | ref | u_prev
  mpcqp::Mapped<uint8_t> stage_out;  // u0 | X | U | status | iters | active
  hipStream_t stage_stream = nullptr;
  // the guess block of the warm B = 1 calls (mpcqp_stage_guess): 2 x N doubles, then guess_passes (i32)
  mpcqp::Mapped<double> stage_guess;
  bool serve_warm = false;  // the kind of the live server wave: k_serve_warm (else k_serve)
  // the B = 1 server: mailbox, sequence number, a server kernel enqueued
  mpcqp::Mapped<mpcqp::ServeBox> serve_box;
  uint32_t serve_seq = 0;
  bool serve_live = false;
  bool serve_broken = false;  // a request went unanswered (30 s): the workspace refuses B = 1 requests
  int serve_fault = 0;        // mpcqp_debug_serve_fault: 1 = refuse the next server launch
  std::chrono::steady_clock::time_point serve_last;  // the last completed request (host clock)
  // guards the server fields above: held by mpcqp_solve_served for its whole call, by set_params /
  // destroy around their stop, and try-locked by another workspace's served call that would stop this
  // workspace's wave (it skips the stop while this one is busy)
  std::mutex serve_mu;
  // two QPs per wave for N <= 15 (MPCQP_PAIR_*, mpcqp_set_pairing)
  int pairing = MPCQP_PAIR_AUTO;
  int cus = 0;  // the device's compute units (queried once at mpcqp_create; 0 if unknown)
  // per-QP parameter classes (mpcqp_set_classes): the device table of n_classes blocks
  mpcqp_params* dclasses = nullptr;
  int n_classes = 0;
  // the table's blocks on the host (mpcqp_swarm_loop_mixed checks every class's dt against the swarm's)
  std::vector<mpcqp_params> hclasses;
  // mpcqp_fleet_loop_mixed (on the nominal workspace): 2 K blocks {nominal[c], relaxed[c]} for
  // dloop_cap classes, filled from the two class tables by a kernel on the launch stream at every call
  mpcqp_params* dloop_classes = nullptr;
  int dloop_cap = 0;
  // mpcqp_set_class_pairing: mixed launches pair within classes; the slot table (2 x max_batch entries),
  // allocated there and written by k_class_slots on the launch stream
  bool class_pairing = false;
  int32_t* dslots = nullptr;
  // mpcqp_launch_info: the last solver launch recorded here {MPCQP_LAUNCH_*, QPs (vehicles) per wave,
  // workgroups, B or V}; host bookkeeping, written by launched_as() and cleared by mpcqp_set_params
  int32_t last_launch[4] = {MPCQP_LAUNCH_NONE, 0, 0, 0};
  // workgroups < 0: count / per_wave rounded up (a class-paired launch runs the slot table's grid instead)
  void launched_as(int kind, int per_wave, int count, int workgroups = -1) {
    last_launch[0] = kind;
    last_launch[1] = per_wave;
    last_launch[2] = workgroups >= 0 ? workgroups : (count + per_wave - 1) / per_wave;
    last_launch[3] = count;
  }
  void no_launch() { last_launch[0] = last_launch[1] = last_launch[2] = last_launch[3] = 0; }
};

namespace mpcqp {
// The fused loops (mpcqp_fleet.hip).  fused_loop: the member `which` (loop, loop_mixed, loop_warm, ...) of
// the horizon that both workspaces' parameter blocks run, or nullptr (another kernel family, debug
// mode, not compiled in, or the two differ).  enqueue_fused_loop: one launch of it after the caller's
// checks -- both builds invalidated, the parameter blocks stored on the stream (L.cls: the two class
// tables, else the workspaces' own blocks; L.P is set here), the longest-first dispatch order when the
// vehicles outnumber the wave slots (L.tr.order is set here), pairing under use_pairs where may_pair
// (the plain loop; the warm loops hand in L.tr.pair themselves), the launch, its record on `nominal` as
// `kind` (MPCQP_LAUNCH_*, mpcqp_launch_info), and `name` in its launch error.
fleet_loop_t fused_loop(const mpcqp_ws* nominal, const mpcqp_ws* relaxed, fleet_loop_t HorizonKernels::*which);
int enqueue_fused_loop(mpcqp_ws* nominal, mpcqp_ws* relaxed, fleet_loop_t loop, const char* name, int kind,
                       bool may_pair, LoopLaunch L, hipStream_t s);
// The mixed loops' class tables (mpcqp_fleet_loop_mixed, mpcqp_swarm_loop_mixed[_warm]; mpcqp_fleet.hip).
// check_loop_classes: MPCQP_E_STATE, the message under `who`, unless both workspaces hold a table of the
// same K >= 1; writes nothing.  grow_loop_classes: nominal->dloop_classes for nominal->n_classes classes,
// allocated outside any capture (MPCQP_E_STATE inside one).
int check_loop_classes(const mpcqp_ws* nominal, const mpcqp_ws* relaxed, const char* who);
int grow_loop_classes(mpcqp_ws* nominal, hipStream_t s);
// two QPs (vehicles) per wave for a warm launch (mpcqp_solve_warm, mpcqp_fleet_loop_warm[_carry],
// mpcqp_swarm_loop_warm)?  Only
// under MPCQP_PAIR_ON and where the paired kernels exist: MPCQP_PAIR_AUTO keeps warm launches at one per
// wave.  Defined in mpcqp.hip.
bool use_pairs_warm(const mpcqp_ws* ws);
// allocate ws->model / ws->state (max_batch QPs) if requested and not yet there; refuses to allocate
// on a capturing stream (the first use must run outside a capture); defined in mpcqp.hip
int ensure_buffers(mpcqp_ws* ws, bool model, bool state, hipStream_t s);
// the solver-state buffer is read or written: the long-horizon kernels' workspace, debug state
inline bool needs_state(const mpcqp_params& p) { return wide_solve(p) || p.debug_state != 0; }
// the stepped fleet's buffers (k_fleet_build writes the models; mpcqp_fleet.hip), before a capture
int fleet_buffers(mpcqp_ws* nominal, mpcqp_ws* relaxed, hipStream_t s);
// One captured step, replayed `steps` times (mpcqp_fleet.hip; the stepped fleet and swarm): waits on
// the caller's stream, runs `prepare` outside the capture, captures step(s2) on a private stream,
// replays it, orders the caller's stream after the replays and waits for them.  `what` ("fleet",
// "swarm") names the caller in the "<what> graph setup / replay" errors.
int replay_graph(const char* what, hipStream_t user, int steps, const std::function<int()>& prepare,
                 const std::function<int(hipStream_t)>& step);
}  // namespace mpcqp
