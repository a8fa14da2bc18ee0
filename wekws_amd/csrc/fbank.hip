// The fbank extractor: instantiations of fbank_kernel (fbank.hip.h), the handle and its C entry points.  (The dithered instantiations
// and their entry points: fbank_dither.hip.)
#include <new>
#include <vector>

#include "model.h"

namespace wekws {
int* fbank_last_launch() {
  static thread_local int rec[8];
  return rec;
}
}  // namespace wekws

// fbank of float or int16 samples
template <class S>
static int fbank_compute(wekws_hip_fbank* f, const S* pcm, int B, int nsamp, float* feats, int resident, void* stream_) {
  if (!f || !pcm || !feats) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  if (B < 0 || nsamp < 0) return fail(WEKWS_HIP_EINVAL, "B=%d nsamp=%d", B, nsamp);
  const int nf = wekws_hip_fbank_num_frames(f, nsamp);
  if (B == 0 || nf == 0) return WEKWS_HIP_OK;
  DeviceGuard guard(f->device);
  const int rc = wekws::launch_fbank<S>(f->fp, pcm, B, nsamp, nf, feats, resident, static_cast<hipStream_t>(stream_));
  if (rc) return fail(rc, "fbank launch failed: %s", hipGetErrorString(hipGetLastError()));
  return WEKWS_HIP_OK;
}

extern "C" {

int wekws_hip_fbank_create(const wekws_hip_fbank_cfg* cfg, int device, wekws_hip_fbank** out) {
  if (!cfg || !out) return fail(WEKWS_HIP_EINVAL, "NULL argument");
  *out = nullptr;
  if (cfg->num_bins <= 0 || cfg->num_bins > wekws::kFbankMaxBins || cfg->sample_rate <= 0 || cfg->frame_length <= 0 ||
      cfg->frame_shift <= 0 || cfg->frame_length > wekws::kFbankMaxFft)
    return fail(WEKWS_HIP_EINVAL, "fbank cfg out of range");
  if (cfg->window != WEKWS_HIP_WINDOW_HAMMING && cfg->window != WEKWS_HIP_WINDOW_POVEY)
    return fail(WEKWS_HIP_EINVAL, "fbank window %d", cfg->window);
  if (cfg->frame_length <= 64)
    // (the reference would transform 64 points or fewer; frames that short -- 4 ms at 16 kHz -- have no recipe, and the
    // mel slots of a 512-point spectrum sampled every 8th bin or sparser are not laid out for it)
    return fail(WEKWS_HIP_EUNSUPPORTED, "fbank frame_length %d: frames of 65 .. 512 samples are built", cfg->frame_length);
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(WEKWS_HIP_EDEVICE, "device %d of %d", device, ndev);
  DeviceGuard guard(device);
  if (!guard.ok) return fail(WEKWS_HIP_EDEVICE, "hipSetDevice(%d)", device);
  wekws_hip_fbank* f = new (std::nothrow) wekws_hip_fbank();
  if (!f) return fail(WEKWS_HIP_ENOMEM, "host allocation");
  f->device = device;
  std::vector<float> tables;
  const int empty = wekws::fbank_build_tables(cfg->num_bins, cfg->sample_rate, cfg->frame_length, cfg->frame_shift, cfg->window,
                                              &f->fp, &tables);
  if (empty >= 0) {                                           // (the reference's constructor CHECK-fails: fbank.h:81)
    delete f;
    return fail(WEKWS_HIP_EINVAL, "fbank: mel filter %d of %d covers no FFT bin (sample_rate %d, frame_length %d): fewer bins", empty,
                cfg->num_bins, cfg->sample_rate, cfg->frame_length);
  }
  hipError_t e = hipMalloc(&f->d_tables, tables.size() * sizeof(float));
  if (e == hipSuccess) e = hipMemcpy(f->d_tables, tables.data(), tables.size() * sizeof(float), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (f->d_tables) (void)hipFree(f->d_tables);
    delete f;
    return fail(WEKWS_HIP_EDEVICE, "fbank table upload: %s", hipGetErrorString(e));
  }
  f->fp.tables = f->d_tables;
  f->resident_f32 = wekws::fbank_resident_groups<float>(f->fp);
  f->resident_i16 = wekws::fbank_resident_groups<int16_t>(f->fp);
  f->resident_dither_f32 = wekws::fbank_dither_resident(f->fp, 4);
  f->resident_dither_i16 = wekws::fbank_dither_resident(f->fp, 2);
  *out = f;
  return WEKWS_HIP_OK;
}

void wekws_hip_fbank_destroy(wekws_hip_fbank* f) {
  if (!f) return;
  DeviceGuard guard(f->device);
  if (f->d_tables) (void)hipFree(f->d_tables);
  delete f;
}

int wekws_hip_fbank_num_frames(const wekws_hip_fbank* f, int nsamp) {
  if (!f || nsamp < f->fp.frame_length) return 0;
  return 1 + (nsamp - f->fp.frame_length) / f->fp.frame_shift;  // fbank.h:141-142
}

int wekws_hip_fbank_compute(wekws_hip_fbank* f, const float* pcm, int B, int nsamp, float* feats, void* stream_) {
  return fbank_compute(f, pcm, B, nsamp, feats, f ? f->resident_f32 : 0, stream_);
}
int wekws_hip_fbank_compute_i16(wekws_hip_fbank* f, const int16_t* pcm, int B, int nsamp, float* feats, void* stream_) {
  return fbank_compute(f, pcm, B, nsamp, feats, f ? f->resident_i16 : 0, stream_);
}

}  // extern "C"
