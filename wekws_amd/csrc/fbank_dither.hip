// The dithered fbank extractor: the DITHER instantiations of the fbank kernel (fbank.hip.h, noise from philox.hip.h), their entry
// points, and wekws_hip_dither_noise -- the normal field those kernels add, written out (the bridge to the oracle).
// Built with -fno-slp-vectorize (Makefile): the generator's scalar f32 chains must stay scalar (pk_safe.hip.h).
#include <cmath>

#include "model.h"

namespace wekws {

template <typename S>
static auto fbank_dither_kern(int rounds) {
  return rounds == 1 ? fbank_dither_kernel<1, S> : rounds == 2 ? fbank_dither_kernel<2, S> : fbank_dither_kernel<3, S>;
}

// workgroups of one resident round of the dithered kernel (its register count is its own): fbank_resident_groups' rule
template <typename S>
static int fbank_dither_resident_of(const FbankParams& P) {
  const int rounds = (P.nslots + 63) / 64;
  if (rounds < 1 || rounds > 3) return 0;
  const size_t lds = size_t(kFbankWaves * kFbankFW * kFbankStrip) * sizeof(float);
  int per_cu = 0, dev = 0;
  hipDeviceProp_t prop;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fbank_dither_kern<S>(rounds), 64 * kFbankWaves, lds) == hipSuccess &&
      hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && per_cu > 0)
    return per_cu * prop.multiProcessorCount;
  return 256 * 4;
}

int fbank_dither_resident(const FbankParams& P, int sample_bytes) {
  return sample_bytes == 4 ? fbank_dither_resident_of<float>(P) : fbank_dither_resident_of<int16_t>(P);
}

template <typename S>
static int launch_fbank_dither(const FbankParams& P, const S* pcm, int B, int nsamp, int nframes, float* feats, int resident,
                               const FbankDither& D, hipStream_t stream) {
  const int rounds = (P.nslots + 63) / 64;
  if (rounds < 1 || rounds > 3) return -4;
  const size_t lds = size_t(kFbankWaves * kFbankFW * kFbankStrip) * sizeof(float);
  const int64_t grid = fbank_grid(int64_t(B) * nframes, resident);
  {
    const int v[8] = {rounds, int(sizeof(S)), int(fbank_pair_ok(nsamp, P.frame_shift, P.frame_length, pcm)), int(grid), resident, B, nsamp, nframes};
    for (int i = 0; i < 8; ++i) fbank_last_launch()[i] = v[i];
  }
  hipLaunchKernelGGL(fbank_dither_kern<S>(rounds), dim3(unsigned(grid)), dim3(64 * kFbankWaves), lds, stream, P, pcm, B, nsamp, nframes,
                     feats, D);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

// One thread per (row, frame, Philox block): the four normals of the block go to the samples philox.hip.h maps them to.
constexpr int kNoiseBlocks = 128;   // blocks of a frame of up to 512 samples
__global__ __launch_bounds__(256) void dither_noise_kernel(uint64_t seed, int64_t first_row, int64_t total, int nframes, int frame_length,
                                                           float* __restrict__ out) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t >= total) return;
  const int64_t g = t / kNoiseBlocks;                        // frame of the call
  const int blk = int(t - g * kNoiseBlocks);
  const int64_t b = g / nframes;
  const int fr = int(g - b * nframes);
  const int n = (blk & 63) + 128 * (blk >> 6);               // the block serves the sample pairs n and n + 64
  if (2 * n >= frame_length) return;
  PhiloxDither G;
  G.init(seed);
  float2 z[2];
  G.block(n, fr, first_row + b, z[0], z[1]);
  float* const row = out + g * frame_length;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int i = 2 * (n + 64 * h);
    if (i < frame_length) row[i] = z[h].x;
    if (i + 1 < frame_length) row[i + 1] = z[h].y;
  }
}

}  // namespace wekws

template <class S>
static int fbank_compute_dither(wekws_hip_fbank* f, const S* pcm, int B, int nsamp, float* feats, float dither, uint64_t seed,
                                int64_t first_row, int resident, void* stream_) {
  if (!f || !pcm || !feats) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || nsamp < 0) return fail(WEKWS_HIP_EINVAL, "B=%d nsamp=%d", B, nsamp);
  if (!(dither >= 0.f) || !std::isfinite(dither)) return fail(WEKWS_HIP_EINVAL, "dither %g: a finite value >= 0", double(dither));
  const int nf = wekws_hip_fbank_num_frames(f, nsamp);
  if (B == 0 || nf == 0) return WEKWS_HIP_OK;
  DeviceGuard guard(f->device);
  const wekws::FbankDither D{dither, seed, first_row};
  const int rc = wekws::launch_fbank_dither<S>(f->fp, pcm, B, nsamp, nf, feats, resident, D, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "fbank launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

extern "C" {

int wekws_hip_fbank_compute_dither(wekws_hip_fbank* f, const float* pcm, int B, int nsamp, float* feats, float dither, uint64_t seed,
                                   int64_t first_row, void* stream_) {
  if (dither == 0.f) return wekws_hip_fbank_compute(f, pcm, B, nsamp, feats, stream_);     // the plain kernel: its bits
  return fbank_compute_dither(f, pcm, B, nsamp, feats, dither, seed, first_row, f ? f->resident_dither_f32 : 0, stream_);
}

int wekws_hip_fbank_compute_dither_i16(wekws_hip_fbank* f, const int16_t* pcm, int B, int nsamp, float* feats, float dither,
                                       uint64_t seed, int64_t first_row, void* stream_) {
  if (dither == 0.f) return wekws_hip_fbank_compute_i16(f, pcm, B, nsamp, feats, stream_);
  return fbank_compute_dither(f, pcm, B, nsamp, feats, dither, seed, first_row, f ? f->resident_dither_i16 : 0, stream_);
}

int wekws_hip_dither_noise(uint64_t seed, int64_t first_row, int B, int nframes, int frame_length, float* out, void* stream_) {
  if (B < 0 || nframes < 0 || frame_length < 1 || frame_length > wekws::kFbankMaxFft)
    return fail(WEKWS_HIP_EINVAL, "B=%d nframes=%d frame_length=%d (need 1 <= frame_length <= %d)", B, nframes, frame_length,
                wekws::kFbankMaxFft);
  if (B == 0 || nframes == 0) return WEKWS_HIP_OK;
  if (!out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  const int64_t total = int64_t(B) * nframes * wekws::kNoiseBlocks;
  if ((total + 255) / 256 > 0x7fffffffLL) return fail(WEKWS_HIP_EINVAL, "dither_noise: too many frames for one launch");
  hipLaunchKernelGGL(wekws::dither_noise_kernel, dim3(unsigned((total + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream_), seed,
                     first_row, total, nframes, frame_length, out);
  if (hipGetLastError() != hipSuccess) return fail(-3, "dither_noise launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

}  // extern "C"
