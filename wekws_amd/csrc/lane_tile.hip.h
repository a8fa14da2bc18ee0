// The LANE-MAJOR REGISTER TILE of the register-resident kernels (ds256_g16 / ds256_g32: 16 waves, DS-TCN h256; mdtc_g4 / ds64_g4:
// C / 16 waves, the small recipes): wave w owns output channels 16 w .. 16 w + 15 for all frames in the accumulator layout of
// the 1x1 convolutions, MFMA column 16 tt + l holds frame NT l + tt (- off).  What every such kernel uses of that layout lives
// here, once: the DPP taps of the depthwise convolutions (with and without a context tile), the scale + split of their outputs
// to the operand planes, the whole-lane runs and tails of the cache slices, and the K step of the matrix products.  What
// the two 4-wave kernels share on top of these: g4_tile.hip.h.
#pragma once
#include <utility>

#include "conv_stack_f16.hip.h"

namespace wekws {

// o += w * x[lane - S] for the lanes whose source stays inside their 16-lane row (the others keep o)
template <int S>
__device__ __forceinline__ void g16_fmac_shr(float& o, float x, float w) {
  static_assert(S >= 1 && S <= 15, "row shift");
#define G16_SHR(n) if constexpr (S == n) asm("v_fmac_f32_dpp %0, %1, %2 row_shr:" #n " row_mask:0xf bank_mask:0xf" : "+v"(o) : "v"(x), "v"(w));
  G16_SHR(1) G16_SHR(2) G16_SHR(3) G16_SHR(4) G16_SHR(5) G16_SHR(6) G16_SHR(7) G16_SHR(8)
  G16_SHR(9) G16_SHR(10) G16_SHR(11) G16_SHR(12) G16_SHR(13) G16_SHR(14) G16_SHR(15)
#undef G16_SHR
}
// Frame layout of the register-resident tile (round 3, second version): MFMA column n = 16 tt + l (tile tt, lane l of the
// 16-lane row) holds FRAME  f(n) = NT l + tt  -- every lane owns NT CONSECUTIVE frames, one per register.  The matrix
// products never look at what a column means (columns are independent), so the permutation costs nothing there; it only
// shows where frames are named: the feature staging, the depthwise taps, the cache slices and the classifier tile.
//   * a tap s frames back, s = q NT + m: register tt - m of the lane q places to the left (tt >= m), else register
//     tt - m + NT of the lane q + 1 places to the left: ONE v_fmac_f32_dpp row_shr per tap and output (the first version, frame
//     = 16 tt + l, needed a row_shr on one tile plus a row_shl on the tile before: 13 instead of 7 DPP operations per
//     output -- and a DPP operation costs 3.3 SIMD cycles at four waves per SIMD against 2.3 for a plain v_fmac,
//     tools/probe/valu_rate.hip), a plain FMA when q = 0, nothing when the lane shift leaves the 16-lane row (left context
//     = zeros, bound_ctrl off);
//   * the slice of the streaming cache a block hands over is pad = 7 d frames = whole lanes when NT | T: 28 contiguous
//     bytes per lane and channel (dwordx4 + dwordx3) instead of 4-byte stores.
template <int S, int TT_, int NT, int R_>
__device__ __forceinline__ void g16_tap(float& o, const f32x4 (&hv)[NT], float w) {
  constexpr int Q = S / NT, M = S % NT;
  constexpr int REG = TT_ >= M ? TT_ - M : TT_ - M + NT;
  constexpr int SH = TT_ >= M ? Q : Q + 1;
  if constexpr (SH == 0) o = fmaf(w, hv[REG][R_], o);
  else if constexpr (SH <= 15) g16_fmac_shr<SH>(o, hv[REG][R_], w);
}
template <int S, int NT, int R_, int... TTs>
__device__ __forceinline__ void g16_tap_tiles(float (&o)[NT], const f32x4 (&hv)[NT], float w, std::integer_sequence<int, TTs...>) {
  (g16_tap<S, TTs, NT, R_>(o[TTs], hv, w), ...);
}

// ---- calls WITH an incoming cache (round 5).  The left context of a block -- the last `pad` frames of its input in the call
// before, its slice of the streaming cache (tcn.py:45-53) -- continues the lane-major tile to the left: frame g < 0 belongs to
// "lane" floor(g / NT) < 0.  It is kept in a second register tile cx whose lane p holds lane p - 16 (only the last
// ceil(pad / NT) lanes are non-zero), so the source of a tap that leaves the 16-lane row to the left is cx, SH lanes back =
// 16 - SH lanes FORWARD in cx: one more v_fmac_f32_dpp, row_shl, for exactly the lanes the row_shr left untouched (bound_ctrl
// off: a lane whose source is outside the row is disabled).  cx shares its registers with the accumulators (dead outside the
// matrix phase and the epilogue).
// o += w * x[lane + S] for the lanes whose source stays inside their 16-lane row (the others keep o)
template <int S>
__device__ __forceinline__ void g16_fmac_shl(float& o, float x, float w) {
  static_assert(S >= 1 && S <= 15, "row shift");
#define G16_SHL(n) if constexpr (S == n) asm("v_fmac_f32_dpp %0, %1, %2 row_shl:" #n " row_mask:0xf bank_mask:0xf" : "+v"(o) : "v"(x), "v"(w));
  G16_SHL(1) G16_SHL(2) G16_SHL(3) G16_SHL(4) G16_SHL(5) G16_SHL(6) G16_SHL(7) G16_SHL(8)
  G16_SHL(9) G16_SHL(10) G16_SHL(11) G16_SHL(12) G16_SHL(13) G16_SHL(14) G16_SHL(15)
#undef G16_SHL
}
// PART 0: the tile's share of the tap (the lanes whose source stays in the row), PART 1: the context's share (the others).  A
// tap's two instructions on one output depend on each other through the accumulator: they are issued as two passes over the NT
// outputs, never back to back.
template <int S, int TT_, int NT, int R_, int PART>
__device__ __forceinline__ void g16_tapc(float& o, const f32x4 (&hv)[NT], const f32x4 (&cx)[NT], float w) {
  constexpr int Q = S / NT, M = S % NT;
  constexpr int REG = TT_ >= M ? TT_ - M : TT_ - M + NT;
  constexpr int SH = TT_ >= M ? Q : Q + 1;
  static_assert(SH <= 15, "the context is one 16-lane row: NT >= 4 for paddings up to 56 frames");
  if constexpr (SH == 0) {
    if constexpr (PART == 0) o = fmaf(w, hv[REG][R_], o);
  } else if constexpr (PART == 0) {
    g16_fmac_shr<SH>(o, hv[REG][R_], w);
  } else {
    g16_fmac_shl<16 - SH>(o, cx[REG][R_], w);
  }
}
template <int S, int NT, int R_, int... TTs>
__device__ __forceinline__ void g16_tapc_tiles(float (&o)[NT], const f32x4 (&hv)[NT], const f32x4 (&cx)[NT], float w,
                                               std::integer_sequence<int, TTs...>) {
  (g16_tapc<S, TTs, NT, R_, 0>(o[TTs], hv, cx, w), ...);
  (g16_tapc<S, TTs, NT, R_, 1>(o[TTs], hv, cx, w), ...);
}

typedef float g16_f32x2 __attribute__((ext_vector_type(2)));
typedef _Float16 g16_f16x2 __attribute__((ext_vector_type(2)));

// scale + split of TWO depthwise outputs (channel rows 2 p and 2 p + 1 of one frame) into one packed hi and one packed lo
// register: t = v s (exact, s is a power of two), hi = fp16(t), lo = fp16(t - hi) -- split16s(), two at a time with
// v_cvt_pk_f16_f32: 8 vector operations per output pair, none of them slow.  (The first version used the
// mixed-precision FMAs, v_fma_mixlo / mixhi_f16 and v_fma_mix_f32, three per output: tools/probe/valu_rate.hip measures
// 6.0 SIMD cycles for one of those at four waves per SIMD against 1.9 for a v_fma_f32 and 3.3 for a packed operation --
// the split was 36 % of the depthwise phase.)  Same roundings, same bits.
// RELU: the depthwise output passes a ReLU first (DS-TCN, tcn.py:102-108; MDTC's has none, mdtc.py:55-58).
template <bool SPLIT, bool RELU = true>
__device__ __forceinline__ void g16_split_pair(float v0, float v1, float s, unsigned& ph, unsigned& pl) {
  const float t0 = (RELU ? fmaxf(v0, 0.f) : v0) * s, t1 = (RELU ? fmaxf(v1, 0.f) : v1) * s;
  const g16_f16x2 h = __builtin_convertvector(g16_f32x2{t0, t1}, g16_f16x2);
  ph = __builtin_bit_cast(unsigned, h);
  if constexpr (SPLIT) {
    const float d0 = t0 - static_cast<float>(h[0]), d1 = t1 - static_cast<float>(h[1]);
    pl = __builtin_bit_cast(unsigned, __builtin_convertvector(g16_f32x2{d0, d1}, g16_f16x2));
  }
}

// Depthwise conv + folded BN [+ ReLU] + scale / split of the channel-row pair (2 P_, 2 P_ + 1) of the lane's four, all NT
// frames of the lane at once: 2 NT independent accumulators per tap, so consecutive instructions never depend on one
// another.  Taps + bias of a channel: one REC-float record {w0 .. w[KT - 1], bias, padding} (BlockDesc::dw_pk), read as 16-byte
// LDS broadcasts; tap j multiplies the frame (KT - 1 - j) dilations back, j ascending like the reference's (and the LDS-tile
// kernels') sum.  CTX (an incoming cache): the taps that leave the 16-lane row continue in the context tile.
//   DS-TCN (tcn.py:102-109): KT = 8, REC = 12, RELU; PRIO (the 16-wave kernel): a wave that is ahead steps back, see its matrix phase.
//   MDTC (mdtc.py:55-58): KT = 5, REC = 8, no ReLU.
template <int J, int N>
__device__ __forceinline__ float dw_rec(const float4 (&q)[N]) {
  return J % 4 == 0 ? q[J / 4].x : J % 4 == 1 ? q[J / 4].y : J % 4 == 2 ? q[J / 4].z : q[J / 4].w;
}
template <int KT, int REC, bool RELU, bool PRIO, int D, int P_, int NT, bool SPLIT, bool CTX, int... Js>
__device__ __forceinline__ void dw_pair(const f32x4 (&hv)[NT], const f32x4 (&cx)[NT], const float* taps_o0, float sa, char* pst, int lo_off,
                                        std::integer_sequence<int, Js...>) {
  const float4* src = reinterpret_cast<const float4*>(taps_o0 + 2 * P_ * REC);
  float4 a[REC / 4], b[REC / 4];
#pragma unroll
  for (int i = 0; i < REC / 4; ++i) a[i] = src[i];
#pragma unroll
  for (int i = 0; i < REC / 4; ++i) b[i] = src[REC / 4 + i];
  constexpr auto tiles = std::make_integer_sequence<int, NT>{};
  constexpr int RA = 2 * P_, RB = 2 * P_ + 1;
  float oa[NT], ob[NT];
  if constexpr (PRIO) __builtin_amdgcn_s_setprio(P_ == 0 ? 3 : 1);
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) { oa[tt] = dw_rec<KT>(a); ob[tt] = dw_rec<KT>(b); }
  if constexpr (CTX)
    ((g16_tapc_tiles<(KT - 1 - Js) * D, NT, RA>(oa, hv, cx, dw_rec<Js>(a), tiles), g16_tapc_tiles<(KT - 1 - Js) * D, NT, RB>(ob, hv, cx, dw_rec<Js>(b), tiles)), ...);
  else
    ((g16_tap_tiles<(KT - 1 - Js) * D, NT, RA>(oa, hv, dw_rec<Js>(a), tiles), g16_tap_tiles<(KT - 1 - Js) * D, NT, RB>(ob, hv, dw_rec<Js>(b), tiles)), ...);
  if constexpr (PRIO) __builtin_amdgcn_s_setprio(P_ == 0 ? 2 : 0);
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    // the pair's two halves of column 16 tt + l15: one 4-byte store per plane (waiting for the other pair to make it an
    // 8-byte store holds 2 NT registers through the second pair's taps: scratch -- the kernels are at the 128-register limit)
    unsigned ph, pl;
    g16_split_pair<SPLIT, RELU>(oa[tt], ob[tt], sa, ph, pl);
    *reinterpret_cast<unsigned*>(pst + tt * 256 + P_ * 4) = ph;
    if constexpr (SPLIT) *reinterpret_cast<unsigned*>(pst + lo_off + tt * 256 + P_ * 4) = pl;
  }
}
template <int KT, int REC, bool RELU, bool PRIO, int D, int NT, bool SPLIT, bool CTX>
__device__ __forceinline__ void dw_rows(const f32x4 (&hv)[NT], const f32x4 (&cx)[NT], const float* taps_o0, float sa, char* pst, int lo_off) {
  dw_pair<KT, REC, RELU, PRIO, D, 0, NT, SPLIT, CTX>(hv, cx, taps_o0, sa, pst, lo_off, std::make_integer_sequence<int, KT>{});
  dw_pair<KT, REC, RELU, PRIO, D, 1, NT, SPLIT, CTX>(hv, cx, taps_o0, sa, pst, lo_off, std::make_integer_sequence<int, KT>{});
}
// the DS-TCN rows (k = 8; ds256_g16, ds64_g4) and the MDTC rows (k = 5; mdtc_g4); without CTX there is no context tile
template <int D, int NT, bool SPLIT, bool CTX = false>
__device__ __forceinline__ void g16_dw_rows(const f32x4 (&hv)[NT], const f32x4 (&cx)[NT], const float* taps_o0, float sa, char* pst, int lo_off) {
  dw_rows<8, 12, true, true, D, NT, SPLIT, CTX>(hv, cx, taps_o0, sa, pst, lo_off);
}
template <int D, int NT, bool SPLIT>
__device__ __forceinline__ void g16_dw_rows(const f32x4 (&hv)[NT], const float* taps_o0, float sa, char* pst, int lo_off) {
  g16_dw_rows<D, NT, SPLIT, false>(hv, hv, taps_o0, sa, pst, lo_off);
}
template <int D, int NT, bool SPLIT, bool CTX = false>
__device__ __forceinline__ void g4_dw_rows(const f32x4 (&hv)[NT], const f32x4 (&cx)[NT], const float* taps_o0, float sa, char* pst, int lo_off) {
  dw_rows<5, 8, false, false, D, NT, SPLIT, CTX>(hv, cx, taps_o0, sa, pst, lo_off);
}
template <int D, int NT, bool SPLIT>
__device__ __forceinline__ void g4_dw_rows(const f32x4 (&hv)[NT], const float* taps_o0, float sa, char* pst, int lo_off) {
  g4_dw_rows<D, NT, SPLIT, false>(hv, hv, taps_o0, sa, pst, lo_off);
}

// NT consecutive floats from a dword-aligned address into row r of the lane's registers, as wide loads (g16_store_run's twin)
template <int NT>
__device__ __forceinline__ void g16_load_run(const float* src, f32x4 (&cv)[NT], int r) {
  struct __attribute__((packed, aligned(4))) V4 { float v[4]; };
  struct __attribute__((packed, aligned(4))) V3 { float v[3]; };
  if constexpr (NT == 7) {
    const V4 a = *reinterpret_cast<const V4*>(src);
    const V3 c = *reinterpret_cast<const V3*>(src + 4);
    cv[0][r] = a.v[0]; cv[1][r] = a.v[1]; cv[2][r] = a.v[2]; cv[3][r] = a.v[3];
    cv[4][r] = c.v[0]; cv[5][r] = c.v[1]; cv[6][r] = c.v[2];
  } else if constexpr (NT == 4) {
    const V4 a = *reinterpret_cast<const V4*>(src);
    cv[0][r] = a.v[0]; cv[1][r] = a.v[1]; cv[2][r] = a.v[2]; cv[3][r] = a.v[3];
  } else {
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) cv[tt][r] = src[tt];
  }
}

// NT consecutive floats (row r of the lane's registers) to a dword-aligned address, as wide stores
template <int NT>
__device__ __forceinline__ void g16_store_run(float* dst, const f32x4 (&hv)[NT], int r) {
  struct __attribute__((packed, aligned(4))) V4 { float v[4]; };
  struct __attribute__((packed, aligned(4))) V3 { float v[3]; };
  struct __attribute__((packed, aligned(4))) V2 { float v[2]; };
  if constexpr (NT == 7) {
    *reinterpret_cast<V4*>(dst) = V4{{hv[0][r], hv[1][r], hv[2][r], hv[3][r]}};
    *reinterpret_cast<V3*>(dst + 4) = V3{{hv[4][r], hv[5][r], hv[6][r]}};
  } else if constexpr (NT == 4) {
    *reinterpret_cast<V4*>(dst) = V4{{hv[0][r], hv[1][r], hv[2][r], hv[3][r]}};
  } else if constexpr (NT == 2) {
    *reinterpret_cast<V2*>(dst) = V2{{hv[0][r], hv[1][r]}};
  } else {
#pragma unroll
    for (int tt = 0; tt < NT; ++tt) dst[tt] = hv[tt][r];
  }
}

// The last S registers of row r (frames NT l + NT - S .. NT l + NT - 1 of the lane) to S consecutive floats
template <int NT, int S>
__device__ __forceinline__ void g4_store_tail(float* dst, const f32x4 (&hv)[NT], int r) {
  struct __attribute__((packed, aligned(4))) V4 { float v[4]; };
  struct __attribute__((packed, aligned(4))) V3 { float v[3]; };
  struct __attribute__((packed, aligned(4))) V2 { float v[2]; };
  static_assert(S >= 1 && S < NT, "a proper suffix");
  constexpr int F = NT - S;
  if constexpr (S >= 4) {
    *reinterpret_cast<V4*>(dst) = V4{{hv[F][r], hv[F + 1][r], hv[F + 2][r], hv[F + 3][r]}};
    if constexpr (S == 5) dst[4] = hv[F + 4][r];
    if constexpr (S == 6) *reinterpret_cast<V2*>(dst + 4) = V2{{hv[F + 4][r], hv[F + 5][r]}};
  } else if constexpr (S == 3) {
    *reinterpret_cast<V3*>(dst) = V3{{hv[F][r], hv[F + 1][r], hv[F + 2][r]}};
  } else if constexpr (S == 2) {
    *reinterpret_cast<V2*>(dst) = V2{{hv[F][r], hv[F + 1][r]}};
  } else {
    dst[0] = hv[F][r];
  }
}
template <int NT, int S = 1>
__device__ __forceinline__ void g4_store_tail_n(int s, float* dst, const f32x4 (&hv)[NT], int r) {
  if constexpr (S < NT) {
    if (s == S) g4_store_tail<NT, S>(dst, hv, r);
    else g4_store_tail_n<NT, S + 1>(s, dst, hv, r);
  }
}

// One 32-deep K step for one o-tile, B fragments of tile tt + 1 requested before the MFMAs of tile tt.
// FIRST: the accumulators start at zero -- the first MFMA of every tile takes the constant 0 as its C operand instead of
// NT x 4 registers that somebody had to clear.
template <int NT, bool SPLIT, bool FIRST = false>
__device__ __forceinline__ void g16_mfma_step(f32x4 (&acc)[NT], const F16Frag& a, const char* bh, const char* bl) {
  f16x8 vh[2], vl[2];
  vh[0] = *reinterpret_cast<const f16x8*>(bh);
  if constexpr (SPLIT) vl[0] = *reinterpret_cast<const f16x8*>(bl);
#pragma unroll
  for (int tt = 0; tt < NT; ++tt) {
    if (tt + 1 < NT) {
      vh[(tt + 1) & 1] = *reinterpret_cast<const f16x8*>(bh + (tt + 1) * 256);
      if constexpr (SPLIT) vl[(tt + 1) & 1] = *reinterpret_cast<const f16x8*>(bl + (tt + 1) * 256);
    }
    __builtin_amdgcn_sched_barrier(0);
    acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h, vh[tt & 1], FIRST ? f32x4{0.f, 0.f, 0.f, 0.f} : acc[tt], 0, 0, 0);
    if constexpr (SPLIT) {
      acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.h, vl[tt & 1], acc[tt], 0, 0, 0);
      acc[tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a.l, vh[tt & 1], acc[tt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

}  // namespace wekws
