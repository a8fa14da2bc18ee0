// The kernels and the forward of the any-shape path.  See generic.hip.h.
#include "generic.hip.h"

namespace wekws {

enum : int {
  GEN_RELU = 1,        // y = max(., 0)
  GEN_RES_AFTER = 2,   // y = act(.) + R          (tcn.py:60: residual after the ReLU)
  GEN_RES_BEFORE = 4,  // y = act(. + R)          (mdtc.py:117-118: residual before the ReLU)
  GEN_SIGMOID = 8,     // y = sigmoid(.)          (kws_model.py:196-199)
  GEN_ACCUM = 16,      // the product is added to what Y holds (further taps of a dense conv)
  GEN_PARTIAL = 32     // raw partial sums: no bias / epilogue (all taps of a dense conv but the last)
};

// Row (b, t) of X / R / Y sits at base + b * bs + t * rs; W[n][k] at W + n * w_ns + k * w_ks.
struct GenGemm {
  const float* X; int64_t x_bs, x_rs;
  const float* W; int64_t w_ns, w_ks;
  const float* bias;
  const float* R; int64_t r_bs, r_rs;
  float* Y; int64_t y_bs, y_rs;
  int Bn, Tn, K, N, flags;
};

constexpr int kGenTile = 64, kGenK = 16;

// 256 threads = 4 waves; workgroup tile 64 x 64, K in chunks of 16 through LDS; wave w multiplies rows 16 w .. 16 w + 15 by all
// 64 columns with v_mfma_f32_16x16x4_f32 (exact f32 products, f32 accumulate): A operand = lane's (row l % 16, k l / 16), B
// operand = (k l / 16, column l % 16), accumulator register i of lane l = (row 4 (l / 16) + i, column l % 16).
__global__ __launch_bounds__(256) void gen_gemm_kernel(const GenGemm g) {
  __shared__ float xs[kGenK][kGenTile + 4];
  __shared__ float ws[kGenK][kGenTile + 4];
  typedef float gen_f32x4 __attribute__((ext_vector_type(4)));
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, lq = lane >> 4;
  const int64_t M = int64_t(g.Bn) * g.Tn;
  const int64_t m0 = int64_t(blockIdx.x) * kGenTile;
  const int n0 = blockIdx.y * kGenTile;
  // this thread's share of a staged tile: row (tid / 4) of the 64, four consecutive k
  const int lr = tid >> 2, lk = (tid & 3) * 4;
  const int64_t xm = m0 + lr;
  const float* xrow = nullptr;
  if (xm < M) { const int64_t b = xm / g.Tn, t = xm - b * g.Tn; xrow = g.X + b * g.x_bs + t * g.x_rs; }
  const int wn = n0 + lr;
  const float* wrow = wn < g.N ? g.W + int64_t(wn) * g.w_ns : nullptr;
  gen_f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = gen_f32x4{0.f, 0.f, 0.f, 0.f};
  // a thread's four k of a chunk are one 16-byte load where the operand's rows are 16-byte aligned runs (the usual case: row
  // strides and K multiples of four floats); the chunk after the current one is requested before the current one is multiplied
  const bool xvec = g.K % 4 == 0 && ((reinterpret_cast<uintptr_t>(g.X) | uintptr_t(g.x_bs * 4) | uintptr_t(g.x_rs * 4)) & 15) == 0;
  const bool wvec = g.K % 4 == 0 && g.w_ks == 1 && ((reinterpret_cast<uintptr_t>(g.W) | uintptr_t(g.w_ns * 4)) & 15) == 0;
  auto fetch = [&](const float* row, int64_t ks, bool vec, int k0) __attribute__((always_inline)) -> gen_f32x4 {
    gen_f32x4 v = {0.f, 0.f, 0.f, 0.f};
    const int k = k0 + lk;
    if (row && k < g.K) {
      if (vec) v = *reinterpret_cast<const gen_f32x4*>(row + k);
      else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
          if (k + q < g.K) v[q] = row[int64_t(k + q) * ks];
      }
    }
    return v;
  };
  gen_f32x4 xq = fetch(xrow, 1, xvec, 0), wq = fetch(wrow, g.w_ks, wvec, 0);
  for (int k0 = 0; k0 < g.K; k0 += kGenK) {
#pragma unroll
    for (int q = 0; q < 4; ++q) { xs[lk + q][lr] = xq[q]; ws[lk + q][lr] = wq[q]; }
    __syncthreads();
    if (k0 + kGenK < g.K) { xq = fetch(xrow, 1, xvec, k0 + kGenK); wq = fetch(wrow, g.w_ks, wvec, k0 + kGenK); }
#pragma unroll
    for (int k4 = 0; k4 < kGenK; k4 += 4) {
      const float a = xs[k4 + lq][wave * 16 + l15];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, ws[k4 + lq][j * 16 + l15], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int64_t m = m0 + wave * 16 + lq * 4 + i;
    if (m >= M) continue;
    const int64_t b = m / g.Tn, t = m - b * g.Tn;
    float* yrow = g.Y + b * g.y_bs + t * g.y_rs;
    const float* rrow = g.R ? g.R + b * g.r_bs + t * g.r_rs : nullptr;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + j * 16 + l15;
      if (n >= g.N) continue;
      float v = acc[j][i];
      if (g.flags & GEN_ACCUM) v += yrow[n];
      if (!(g.flags & GEN_PARTIAL)) {
        if (g.bias) v += g.bias[n];
        if ((g.flags & GEN_RES_BEFORE) && rrow) v += rrow[n];
        if (g.flags & GEN_RELU) v = nf_relu(v);                // (torch.relu: a NaN stays a NaN -- this path is plain IEEE f32)
        if ((g.flags & GEN_RES_AFTER) && rrow) v += rrow[n];
        if (g.flags & GEN_SIGMOID) v = sigmoidf_(v);
      }
      yrow[n] = v;
    }
  }
}

// Where element (b, c, tau) of a streaming cache sits: conv backbones (B, C, P) with the block's slice at `off`
// (tcn.py:155-165, mdtc.py:250-275): bs = C P, cs = P, ts = 1; FSMN (B, D, P, L), layer index innermost (fsmn.py:495):
// bs = D P L, cs = P L, ts = L, off = layer.
struct GenCacheMap { int64_t bs, cs, ts, off; };

// u[b][tau][c] = tau < pad ? (cache ? cache(b, c, tau) : 0) : h[b][tau - pad][c];  out_cache(b, c, p) = u[b][T + p][c]
__global__ void gen_ctx_kernel(float* __restrict__ u, const float* __restrict__ h, int64_t h_bs, int64_t h_rs,
                               const float* __restrict__ cin, float* __restrict__ cout, GenCacheMap cm, int B, int T, int C, int pad) {
  const int64_t n = int64_t(B) * (pad + T) * C;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int c = int(i % C);
    const int64_t r = i / C;
    const int tau = int(r % (pad + T));
    const int64_t b = r / (pad + T);
    const float v = tau < pad ? (cin ? cin[b * cm.bs + c * cm.cs + tau * cm.ts + cm.off] : 0.f) : h[b * h_bs + int64_t(tau - pad) * h_rs + c];
    u[i] = v;
    if (cout && tau >= T) cout[b * cm.bs + c * cm.cs + int64_t(tau - T) * cm.ts + cm.off] = v;
  }
}

// out[b][t][c] = [ReLU](bias[c] + sum_j w[c][j] u[b][t + j dil][c]),  j = 0 the oldest tap (cross-correlation, like Conv1d)
__global__ void gen_dw_kernel(float* __restrict__ out, const float* __restrict__ u, const float* __restrict__ w,
                              const float* __restrict__ bias, int B, int T, int C, int ks, int dil, int relu) {
  const int pad = (ks - 1) * dil;
  const int64_t n = int64_t(B) * T * C;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int c = int(i % C);
    const int64_t r = i / C;
    const int t = int(r % T);
    const int64_t b = r / T;
    const float* up = u + (b * (pad + T) + t) * C + c;
    const float* wp = w + int64_t(c) * ks;
    float acc = bias ? bias[c] : 0.f;
    for (int j = 0; j < ks; ++j) acc = fmaf(wp[j], up[int64_t(j) * dil * C], acc);
    out[i] = relu ? nf_relu(acc) : acc;
  }
}

// mode 0: y += x;  1: y = x;  2: y = sigmoid(x)
__global__ void gen_add_kernel(float* __restrict__ y, const float* __restrict__ x, int64_t n, int mode) {
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x)
    y[i] = mode == 0 ? y[i] + x[i] : mode == 1 ? x[i] : sigmoidf_(x[i]);
}

// out[b][c] = mean_t h[b][t][c]  (classifier.py:27)  /  h[b][T - 1][c]  (classifier.py:39)
__global__ void gen_pool_kernel(float* __restrict__ out, const float* __restrict__ h, int B, int T, int C, int last) {
  const int64_t n = int64_t(B) * C;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int c = int(i % C);
    const int64_t b = i / C;
    const float* p = h + b * T * C + c;
    if (last) { out[i] = p[int64_t(T - 1) * C]; continue; }
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += p[int64_t(t) * C];
    out[i] = s / float(T);
  }
}

// One step of torch.nn.GRU for all streams: gi = W_ih x_t + b_ih (row (b, t) of a (B T, 3H) matrix), gh = W_hh h + b_hh (B, 3H):
//   r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r gh_n), h' = (1 - z) n + z h   -> hst (B, H) and seq[b][t][:]
__global__ void gen_gru_cell_kernel(const float* __restrict__ gi, const float* __restrict__ gh, float* __restrict__ hst,
                                    float* __restrict__ seq, int B, int T, int H, int t) {
  const int64_t n = int64_t(B) * H;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int u = int(i % H);
    const int64_t b = i / H;
    const float* a = gi + (b * T + t) * 3 * H;
    const float* g = gh + b * 3 * H;
    const float r = 1.f / (1.f + expf(-(a[u] + g[u])));
    const float z = 1.f / (1.f + expf(-(a[H + u] + g[H + u])));
    const float c = tanhf(a[2 * H + u] + r * g[2 * H + u]);
    const float hp = hst[i];
    const float hn = (1.f - z) * c + z * hp;
    hst[i] = hn;
    seq[(b * T + t) * H + u] = hn;
  }
}

// ------------------------------------------------------------------------------------------------------------------------------
// y[r][c] = [ReLU](w[c * ld + c] x[r][c] + bias[c]): the diagonal preprocessing of NoSubsampling (subsampling.py:35-36: the features
// ARE the hidden tile; the diagonal carries a folded CMVN).  Channel by channel like the reference -- through the matrix product
// an Inf in one channel would meet the zeros of every other row (0 * Inf = NaN).
__global__ void gen_diag_kernel(float* __restrict__ y, const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                int64_t rows, int C, int ld, int relu) {
  const int64_t n = rows * C;
  for (int64_t i = int64_t(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += int64_t(gridDim.x) * blockDim.x) {
    const int c = int(i % C);
    const float v = fmaf(w[int64_t(c) * ld + c], x[i], bias[c]);
    y[i] = relu ? nf_relu(v) : v;
  }
}

static int gen_grid(int64_t n) { return int(std::min<int64_t>((n + 255) / 256, 16384)); }

static void gen_gemm(hipStream_t st, const float* X, int64_t x_bs, int64_t x_rs, const float* W, int64_t w_ns, int64_t w_ks,
                     const float* bias, const float* R, int64_t r_bs, int64_t r_rs, float* Y, int64_t y_bs, int64_t y_rs, int Bn,
                     int Tn, int K, int N, int flags) {
  const GenGemm g{X, x_bs, x_rs, W, w_ns, w_ks, bias, R, r_bs, r_rs, Y, y_bs, y_rs, Bn, Tn, K, N, flags};
  const int64_t M = int64_t(Bn) * Tn;
  hipLaunchKernelGGL(gen_gemm_kernel, dim3(unsigned((M + kGenTile - 1) / kGenTile), unsigned((N + kGenTile - 1) / kGenTile)), dim3(256), 0, st, g);
}
// dense rows: Y (M, N) = epilogue(X (M, K) W (N, K)^T + b)
static void gen_linear(hipStream_t st, const float* X, const float* W, const float* bias, const float* R, float* Y, int64_t M, int K,
                       int N, int flags) {
  gen_gemm(st, X, 0, K, W, K, 1, bias, R, 0, N, Y, 0, N, 1, int(M), K, N, flags);
}

// The forward of wekws_hip_forward for a GenericModel (everything but the trailing softmax, which the caller applies).
// ws: gen_workspace_bytes(m, B, T) bytes of scratch.  Returns 0, or -3 if a launch failed.
int generic_forward(const GenericModel& m, const float* x, int B, int T, const float* in_cache, float* y, float* out_cache,
                    char* ws, hipStream_t st, hipError_t* launch_error) {
  auto done = [&]() {                                       // (hipGetLastError resets the sticky error: read once, hand it back)
    const hipError_t e = hipGetLastError();
    if (launch_error) *launch_error = e;
    return e == hipSuccess ? 0 : -3;
  };
  const wekws_hip_desc& d = m.d;
  const int64_t rows = int64_t(B) * T;
  const int C = d.hdim, W = gen_width(d);
  const size_t mat = gen_al(size_t(rows) * W * 4);
  float* hA = reinterpret_cast<float*>(ws);
  float* hB = reinterpret_cast<float*>(ws + mat);
  float* tm = reinterpret_cast<float*>(ws + 2 * mat);
  float* zs = reinterpret_cast<float*>(ws + 3 * mat);
  float* ub = reinterpret_cast<float*>(ws + 4 * mat);
  const BlobLayout L = blob_layout(d);                        // where the tensors lie: blob_layout.h
  const float* w = m.w;
  const int act = d.activation == WEKWS_HIP_ACT_SIGMOID ? GEN_SIGMOID : 0;
  float* h = hA;                                              // the current activation tile (rows, width of the layer)
  float* o = hB;
  auto swap = [&]() { std::swap(h, o); };

  if (d.backbone == WEKWS_HIP_BACKBONE_FSMN) {
    // fsmn.py:462-495 (preprocessing none, identity head: fsmn_ctc.yaml:36-56)
    const int A0 = d.aux[0], A1 = d.aux[1], D = d.num_stack, lo = d.kernel_size, ro = d.stack_size, P = lo - 1 + ro, NL = d.num_layers;
    gen_linear(st, x, w + L.in1_w().off, w + L.in1_b().off, nullptr, h, rows, d.idim, A0, 0);         // in_linear1
    gen_linear(st, h, w + L.in2_w().off, w + L.in2_b().off, nullptr, o, rows, A0, C, GEN_RELU);       // in_linear2 + ReLU
    swap();
    for (int l = 0; l < NL; ++l) {
      const FsmnWeights lw = L.fsmn_layer(l);
      const float *wproj = w + lw.wproj.off, *taps = w + lw.taps.off, *waff = w + lw.waff.off, *baff = w + lw.baff.off;
      gen_linear(st, h, wproj, nullptr, nullptr, tm, rows, C, D, 0);                                  // LinearTransform, no bias
      const GenCacheMap cm{int64_t(D) * P * NL, int64_t(P) * NL, NL, l};
      hipLaunchKernelGGL(gen_ctx_kernel, dim3(gen_grid(int64_t(B) * (P + T) * D)), dim3(256), 0, st, ub, tm, int64_t(T) * D, int64_t(D),
                         in_cache, out_cache, cm, B, T, D, P);
      hipLaunchKernelGGL(gen_dw_kernel, dim3(gen_grid(rows * D)), dim3(256), 0, st, tm, ub, taps, static_cast<const float*>(nullptr), B, T,
                         D, lo + ro, 1, 0);                                                             // memory block (+ identity tap)
      gen_linear(st, tm, waff, baff, nullptr, o, rows, D, C, GEN_RELU);                               // AffineTransform + ReLU
      swap();
    }
    gen_linear(st, h, w + L.out1_w().off, w + L.out1_b().off, nullptr, o, rows, C, A1, 0);            // out_linear1
    gen_linear(st, o, w + L.out2_w().off, w + L.out2_b().off, nullptr, y, rows, A1, d.odim, act);     // out_linear2
    return done();
  }

  // ---- preprocessing: LinearSubsampling1 (subsampling.py:53-57) or the CMVN-only diagonal (preproc_relu = 0)
  if (m.pre_diag)
    hipLaunchKernelGGL(gen_diag_kernel, dim3(gen_grid(rows * C)), dim3(256), 0, st, h, x, w + L.pre_w().off, w + L.pre_b().off, rows, C,
                       d.idim, d.preproc_relu);
  else
    gen_linear(st, x, w + L.pre_w().off, w + L.pre_b().off, nullptr, h, rows, d.idim, C, d.preproc_relu ? GEN_RELU : 0);

  if (d.backbone == WEKWS_HIP_BACKBONE_GRU) {
    const int H = C, NL = d.num_layers;
    float* gh = reinterpret_cast<float*>(reinterpret_cast<char*>(ub) + gen_al(size_t(B) * T * H * 4));   // (ub itself is unused here)
    float* hst = reinterpret_cast<float*>(reinterpret_cast<char*>(gh) + gen_al(size_t(B) * 3 * H * 4));
    for (int l = 0; l < NL; ++l) {
      const GruWeights lw = L.gru_layer(l);
      const float *wih = w + lw.w_ih.off, *whh = w + lw.w_hh.off, *bih = w + lw.b_ih.off, *bhh = w + lw.b_hh.off;
      gen_linear(st, h, wih, bih, nullptr, tm, rows, H, 3 * H, 0);                                    // gi for all steps
      if (in_cache) (void)hipMemcpyAsync(hst, in_cache + size_t(l) * B * H, size_t(B) * H * 4, hipMemcpyDeviceToDevice, st);
      else (void)hipMemsetAsync(hst, 0, size_t(B) * H * 4, st);
      for (int t = 0; t < T; ++t) {
        gen_linear(st, hst, whh, bhh, nullptr, gh, B, H, 3 * H, 0);
        hipLaunchKernelGGL(gen_gru_cell_kernel, dim3(gen_grid(int64_t(B) * H)), dim3(256), 0, st, tm, gh, hst, o, B, T, H, t);
      }
      if (out_cache) (void)hipMemcpyAsync(out_cache + size_t(l) * B * H, hst, size_t(B) * H * 4, hipMemcpyDeviceToDevice, st);
      swap();
    }
  } else {
    const ConvSchedule sched = conv_schedule(d);              // route.h
    const int ks = d.kernel_size, Pc = m.cache_len;
    bool zinit = true;
    for (int i = 0; i < sched.nb; ++i) {
      const ConvBlock blk = sched.block(i);
      const ConvWeights bw = L.block(i);
      const float *wd = w + bw.wd.off, *bd = w + bw.bd.off, *w1 = w + bw.w1.off, *b1 = w + bw.b1.off;
      const int dil = blk.dil, pad = blk.pad;
      const GenCacheMap cm{int64_t(C) * Pc, Pc, 1, blk.cache_off};
      hipLaunchKernelGGL(gen_ctx_kernel, dim3(gen_grid(int64_t(B) * (pad + T) * C)), dim3(256), 0, st, ub, h, int64_t(T) * C, int64_t(C),
                         in_cache, out_cache, cm, B, T, C, pad);
      if (d.backbone == WEKWS_HIP_BACKBONE_DS_TCN) {
        hipLaunchKernelGGL(gen_dw_kernel, dim3(gen_grid(rows * C)), dim3(256), 0, st, tm, ub, wd, bd, B, T, C, ks, dil, 1);
        gen_linear(st, tm, w1, b1, h, o, rows, C, C, GEN_RELU | GEN_RES_AFTER);                       // tcn.py:101-114, :60
      } else if (d.backbone == WEKWS_HIP_BACKBONE_TCN) {
        for (int j = 0; j < ks; ++j) {                                                                 // tap j reads u rows t + j dil
          const bool lastj = j == ks - 1;
          gen_gemm(st, ub + int64_t(j) * dil * C, int64_t(pad + T) * C, C, w1 + j, int64_t(C) * ks, ks, lastj ? b1 : nullptr,
                   lastj ? h : nullptr, int64_t(T) * C, C, o, int64_t(T) * C, C, B, T, C, C,
                   (j ? GEN_ACCUM : 0) | (lastj ? (GEN_RELU | GEN_RES_AFTER) : GEN_PARTIAL));         // W[o][c][j]; tcn.py:75-84, :60
        }
      } else {                                                                                          // MDTC, mdtc.py:95-121
        hipLaunchKernelGGL(gen_dw_kernel, dim3(gen_grid(rows * C)), dim3(256), 0, st, tm, ub, wd, bd, B, T, C, ks, dil, 0);
        gen_linear(st, tm, w1, b1, nullptr, o, rows, C, C, GEN_RELU);
        gen_linear(st, o, w + bw.w2.off, w + bw.b2.off, h, tm, rows, C, C, GEN_RELU | GEN_RES_BEFORE);
        std::swap(tm, o);                                                                               // (the block's output is in `o` again)
        if (blk.zadd) {                                                                                 // end of a stack: mdtc.py:270-273
          hipLaunchKernelGGL(gen_add_kernel, dim3(gen_grid(rows * C)), dim3(256), 0, st, zs, o, rows * C, zinit ? 1 : 0);
          zinit = false;
        }
      }
      swap();
    }
    if (d.backbone == WEKWS_HIP_BACKBONE_MDTC) h = zs;                                                  // the classifier sees the sum of the stack outputs
  }

  // ---- classifier (classifier.py:26-28, :38-40, :63-67) + activation (kws_model.py:196-210)
  if (d.head == WEKWS_HIP_HEAD_LINEAR) {
    gen_linear(st, h, w + L.head_w().off, w + L.head_b().off, nullptr, y, rows, C, d.odim, act);
  } else if (d.head == WEKWS_HIP_HEAD_IDENTITY) {
    hipLaunchKernelGGL(gen_add_kernel, dim3(gen_grid(rows * C)), dim3(256), 0, st, y, h, rows * C, act ? 2 : 1);
  } else {
    const int HH = d.head_hidden;
    float* pooled = tm;                                       // (tm and o are free here)
    hipLaunchKernelGGL(gen_pool_kernel, dim3(gen_grid(int64_t(B) * C)), dim3(256), 0, st, pooled, h, B, T, C, d.head == WEKWS_HIP_HEAD_LAST ? 1 : 0);
    float* hid = o;
    gen_linear(st, pooled, w + L.head_w().off, w + L.head_b().off, nullptr, hid, B, C, HH, GEN_RELU);
    gen_linear(st, hid, w + L.head_w2().off, w + L.head_b2().off, nullptr, y, B, HH, d.odim, act);
  }
  return done();
}

}  // namespace wekws
