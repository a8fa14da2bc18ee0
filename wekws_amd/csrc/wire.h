// Wire encodings (enum wekws_hip_wire, include/wekws_hip.h states the table): how one sample of a stream's bytes becomes one int16
// value.  Host and device, the single definition: wekws_hip_wire_decode on the host and the rate bank's fetch on the device
// (resample.hip.h: ResampleWireChunk) call these functions and nothing else.  Integer arithmetic throughout, except F32: one
// float multiply by 2^15 (exact), one round to nearest even, two clamps -- the same IEEE operations on either side.
#pragma once
#include <stdint.h>

#include <cmath>

#include "../../include/wekws_hip.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define WEKWS_WIRE_FN __host__ __device__ inline
#else
#define WEKWS_WIRE_FN inline
#endif

namespace wekws {

constexpr int kWireCount = 5;

// bytes of one sample; 0: no such encoding
WEKWS_WIRE_FN int wire_sample_bytes(int enc) {
  return enc == WEKWS_HIP_WIRE_S16 ? 2 : enc == WEKWS_HIP_WIRE_F32 ? 4 : (enc >= WEKWS_HIP_WIRE_MULAW && enc <= WEKWS_HIP_WIRE_U8) ? 1 : 0;
}

// ITU-T G.711 mu-law: c the byte as it travels (complemented)
WEKWS_WIRE_FN int wire_mulaw(uint32_t c) {
  const uint32_t u = ~c & 0xFFu;
  const int t = int((((u & 0x0Fu) << 3) + 0x84u) << ((u & 0x70u) >> 4));
  return (u & 0x80u) ? 0x84 - t : t - 0x84;
}
// ITU-T G.711 A-law: c the byte as it travels (even bits inverted)
WEKWS_WIRE_FN int wire_alaw(uint32_t c) {
  const uint32_t a = (c ^ 0x55u) & 0xFFu;
  const int s = int((a & 0x70u) >> 4);
  int t = int((a & 0x0Fu) << 4);
  t += s ? 0x108 : 8;
  if (s > 1) t <<= s - 1;
  return (a & 0x80u) ? t : -t;
}
WEKWS_WIRE_FN int wire_u8(uint32_t c) { return (int(c & 0xFFu) - 128) * 256; }
// unit-scale float: x 2^15 is exact in float32 (an overflow is +-Inf and saturates); rintf rounds half to even on both sides
WEKWS_WIRE_FN int wire_f32(float x) {
  if (x != x) return 0;
  const float r = rintf(x * 32768.0f);
  return int(r < -32768.f ? -32768.f : (r > 32767.f ? 32767.f : r));
}
// one of the single-byte encodings (enc is MULAW, ALAW or U8)
WEKWS_WIRE_FN int wire_byte(int enc, uint32_t c) {
  return enc == WEKWS_HIP_WIRE_MULAW ? wire_mulaw(c) : enc == WEKWS_HIP_WIRE_ALAW ? wire_alaw(c) : wire_u8(c);
}

}  // namespace wekws
