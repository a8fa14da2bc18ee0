// kws_main for the MI355X runtime.  Observable behaviour follows the reference tool
// (runtime/core/bin/kws_main.cc:23-61) so that scripts built around it keep working:
//   kws_main fbank_dim(int) batch_size(int) kws_model_path test_wav_path
//   -> one line per frame:  "frame <index> prob <p0> <p1> ..."   (6 significant digits, like operator<<(float))
// The wav file is decoded, a file whose header rate is not 16000 is resampled to it on the GPU (wekws_hip_resample_*: the
// `resample` step the reference's recipes put in front of the features), its features come from the GPU fbank
// (wenet::FeaturePipeline here), and the spotter is fed
// `batch_size` frames at a time with its streaming cache carried from call to call.  model_path may be the exporter's
// .onnx, an ORT-format .ort, or a packed model (runtime/kws/model_file.h).
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "frontend/feature_pipeline.h"
#include "frontend/wav.h"
#include "kws/keyword_spotting.h"
#include "utils/check.h"

namespace {

struct Options {
  int feature_dim = 0;
  int frames_per_call = 0;
  std::string model, audio;
};

Options ParseCommandLine(int argc, char** argv) {
  if (argc != 5) WEKWS_FATAL() << "Usage: kws_main fbank_dim(int) batch_size(int) kws_model_path test_wav_path";
  Options o;
  o.feature_dim = std::atoi(argv[1]);
  o.frames_per_call = std::atoi(argv[2]);
  o.model = argv[3];
  o.audio = argv[4];
  WEKWS_CHECK(o.feature_dim > 0 && o.frames_per_call > 0) << "fbank_dim and batch_size must be positive integers";
  return o;
}

using Frames = std::vector<std::vector<float>>;

// "frame <n> prob <p...>" for every row, numbered from first_index
void PrintRows(const Frames& rows, size_t first_index) {
  std::string line;
  char num[48];
  for (size_t r = 0; r < rows.size(); ++r) {
    line = "frame " + std::to_string(first_index + r) + " prob";
    for (float p : rows[r]) {
      std::snprintf(num, sizeof(num), " %g", static_cast<double>(p));
      line += num;
    }
    std::puts(line.c_str());
  }
  std::fflush(stdout);
}

constexpr int kModelRate = 16000;

// samples at `rate` -> samples at 16 kHz, float32 in int16 scale as the pipeline takes them (the one-shot float entry point)
std::vector<float> ResampleTo16k(const std::vector<float>& in, int rate) {
  wekws_hip_resample_cfg cfg{};
  cfg.orig_freq = rate;
  cfg.new_freq = kModelRate;
  cfg.lowpass_filter_width = 6;
  cfg.rolloff = 0.99;
  cfg.out_dtype = WEKWS_HIP_RESAMPLE_OUT_F32;
  void* rs = nullptr;
  WEKWS_CHECK(wekws_hip_resample_create(&cfg, &rs) == WEKWS_HIP_OK) << "resampling " << rate << " Hz: " << wekws_hip_last_error();
  const int64_t n_out = wekws_hip_resample_num_samples(rate, kModelRate, static_cast<int64_t>(in.size()));
  WEKWS_CHECK(in.size() <= 0x3fffffff && n_out >= 0 && n_out <= 0x3fffffff) << "file too long to resample in one call";
  std::vector<float> out(static_cast<size_t>(n_out));
  if (n_out == 0) {
    wekws_hip_resample_destroy(rs);
    return out;
  }
  float* d_in = nullptr;
  float* d_out = nullptr;
  WEKWS_CHECK(hipMalloc(reinterpret_cast<void**>(&d_in), in.size() * sizeof(float)) == hipSuccess);
  WEKWS_CHECK(hipMalloc(reinterpret_cast<void**>(&d_out), out.size() * sizeof(float)) == hipSuccess);
  WEKWS_CHECK(hipMemcpy(d_in, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice) == hipSuccess);
  WEKWS_CHECK(wekws_hip_resample_compute(rs, d_in, 1, static_cast<int>(in.size()), nullptr, d_out, static_cast<int>(n_out), nullptr) ==
              WEKWS_HIP_OK)
      << wekws_hip_last_error();
  WEKWS_CHECK(hipMemcpy(out.data(), d_out, out.size() * sizeof(float), hipMemcpyDeviceToHost) == hipSuccess);
  (void)hipFree(d_in);
  (void)hipFree(d_out);
  wekws_hip_resample_destroy(rs);
  return out;
}

}  // namespace

int main(int argc, char** argv) {
  const Options opt = ParseCommandLine(argc, argv);

  // whole file in, as the reference tool does; the pipeline hands frames out batch by batch below
  std::vector<float> samples;
  {
    wenet::WavReader reader(opt.audio);
    WEKWS_CHECK(reader.ok()) << "cannot read " << opt.audio;
    samples.assign(reader.data(), reader.data() + reader.num_samples());
    if (reader.sample_rate() != kModelRate) samples = ResampleTo16k(samples, reader.sample_rate());
  }
  wenet::FeaturePipeline features(wenet::FeaturePipelineConfig(opt.feature_dim, kModelRate));
  features.AcceptWaveform(samples);
  features.set_input_finished();

  wekws::KeywordSpotting spotter(opt.model);
  WEKWS_CHECK(spotter.feature_dim() == opt.feature_dim) << "model expects " << spotter.feature_dim() << "-d features";

  size_t emitted = 0;
  for (bool more = true; more;) {
    Frames chunk, scores;
    more = features.Read(opt.frames_per_call, &chunk);   // false once the pipeline has been drained
    spotter.Forward(chunk, &scores);
    PrintRows(scores, emitted);
    emitted += scores.size();
  }
  return 0;
}
