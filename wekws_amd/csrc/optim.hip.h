// The optimiser step on the device: clip_grad_norm_ (torch/nn/utils/clip_grad.py), the finite test of the reference's training
// loop (wekws/utils/executor.py:58-60) and torch's single-tensor Adam (torch/optim/adam.py), over four flat float32 buffers --
// params, grads, exp_avg, exp_avg_sq -- of n elements each.  The kernels take four base pointers and a length: no tables of
// per-tensor pointers.  Three launches a step (optim_plan.h has the cut and the state block):
//   grad_sumsq_kernel   one workgroup a tile of kOptimTileFloats gradients: 16-byte loads (a scalar tail in the last tile), each
//                       gradient converted to double -- exact, and so is its square -- and added per lane in ascending order,
//                       the 256 lanes merged by one fixed tree through LDS; one double a tile goes to the workspace.
//   clip_fold_kernel    one workgroup folds up to kOptimFoldSeg partials by the same tree; more tiles are first folded
//                       kOptimFoldSeg at a time by a launch of the same kernel.  The last stage takes the square root, decides
//                       whether the step is applied, advances the counters and leaves the coefficient, both bias corrections
//                       (pow in double) and the step size in the state block.
//   adam_apply_kernel   elementwise: reads the state block, then p, g, m, v with 16-byte loads and writes p, m, v with 16-byte
//                       stores (scalars past the last whole float4).  apply == 0: returns before any load of the buffers.
// So the bits of a step are a function of the buffers, the state block and the hyper-parameters alone: no floating-point
// atomics, no dependence on the grid or the CU count.  Nothing synchronises, allocates or reads on the host.
//
// Arithmetic of the update is float32, operation by operation what torch's Adam does to a float32 tensor; sqrt and division are
// the correctly rounded ones (this object is built without fast-math, and hipcc's default keeps both correctly rounded).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "optim_plan.h"

namespace wekws {

// the 256 lanes' values in one fixed order: lane i += lane i + 128, then + 64, ... ; the sum is valid on lane 0
__device__ inline double optim_fold_lanes(double s, double* lds) {
  const int tid = threadIdx.x;
  lds[tid] = s;
  __syncthreads();
#pragma unroll
  for (int off = kOptimThreads / 2; off > 0; off >>= 1) {
    if (tid < off) lds[tid] += lds[tid + off];
    __syncthreads();
  }
  return lds[0];
}

// partial[tile] = sum of g[i]^2 over the tile's floats, in double
__global__ __launch_bounds__(kOptimThreads) void grad_sumsq_kernel(const float* __restrict__ g, int64_t n, double* __restrict__ partial) {
  __shared__ double lds[kOptimThreads];
  constexpr int kLoads = kOptimTileFloats / (4 * kOptimThreads);
  const int tid = threadIdx.x;
  const int64_t base = int64_t(blockIdx.x) * kOptimTileFloats;
  const int cnt = int(n - base < kOptimTileFloats ? n - base : kOptimTileFloats);   // >= 1: the grid is optim_tiles(n)
  const int nv = cnt >> 2, tail = cnt & 3;                     // whole float4s, then up to three scalars (the last tile only)
  const float4* gv = reinterpret_cast<const float4*>(g + base);
  float4 x[kLoads];
#pragma unroll
  for (int k = 0; k < kLoads; ++k) {
    const int i = k * kOptimThreads + tid;
    x[k] = make_float4(0.f, 0.f, 0.f, 0.f);                    // past the tile's end: adds +0.0, nothing is loaded
    if (i < nv) x[k] = gv[i];
  }
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < kLoads; ++k) {
    const double a = double(x[k].x), b = double(x[k].y), c = double(x[k].z), d = double(x[k].w);
    s = fma(a, a, s);
    s = fma(b, b, s);
    s = fma(c, c, s);
    s = fma(d, d, s);
  }
  if (tid < tail) {
    const double a = double(g[base + 4 * nv + tid]);
    s = fma(a, a, s);
  }
  s = optim_fold_lanes(s, lds);
  if (tid == 0) partial[blockIdx.x] = s;
}

// Workgroup x folds rows [x seg, min(nrows, (x + 1) seg)), seg = kOptimFoldSeg.
//   seg_out != NULL                 the first of two stages: seg_out[x] = the sum
//   else norm_out != NULL           one workgroup: *norm_out = float32(sqrt(sum))       (wekws_hip_grad_norm)
//   else                            one workgroup: the state block                       (wekws_hip_clip_adam_step)
__global__ __launch_bounds__(kOptimThreads) void clip_fold_kernel(const double* __restrict__ rows, int nrows, double* __restrict__ seg_out,
                                                                  float* __restrict__ norm_out, OptimState* __restrict__ st, double lr,
                                                                  double beta1, double beta2, double max_norm, int skip_nonfinite) {
  __shared__ double lds[kOptimThreads];
  const int i = blockIdx.x * kOptimFoldSeg + threadIdx.x;
  const double sum = optim_fold_lanes(i < nrows ? rows[i] : 0.0, lds);
  if (threadIdx.x != 0) return;
  if (seg_out) {
    seg_out[blockIdx.x] = sum;
    return;
  }
  const double norm = sqrt(sum);
  const float norm32 = float(norm);
  if (norm_out) {
    *norm_out = norm32;
    return;
  }
  const int finite = isfinite(norm32) ? 1 : 0;
  // clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1 (a NaN stays a NaN, as torch.clamp has it);
  // max_norm = +Inf is "no clipping": exactly 1 whatever the norm
  double coef = 1.0;
  if (max_norm < __builtin_inf()) {
    coef = max_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  const int apply = (finite || !skip_nonfinite) ? 1 : 0;
  st->norm = norm;
  st->norm_f32 = norm32;
  st->finite = finite;
  st->coef = float(coef);
  st->apply = apply;
  if (apply) {
    const int64_t step = st->step + 1;
    const double bc1 = 1.0 - pow(beta1, double(step));
    const double bc2sqrt = sqrt(1.0 - pow(beta2, double(step)));
    st->step = step;
    st->bc1 = bc1;
    st->bc2sqrt = bc2sqrt;
    st->step_size = float(lr / bc1);
    st->bc2sqrt_f32 = float(bc2sqrt);
  } else {
    st->skipped = st->skipped + 1;
  }
}

struct OptimHyper {
  float beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;   // 1 - beta formed in double on the host, as torch does
};

// torch's _single_tensor_adam on one element, with the clip coefficient folded into the gradient
__device__ inline void adam_element(float& p, float g, float& m, float& v, float coef, float step_size, float bc2sqrt,
                                    const OptimHyper& h) {
  const float gt = coef * g + h.weight_decay * p;
  m = h.beta1 * m + h.one_minus_beta1 * gt;
  v = h.beta2 * v + h.one_minus_beta2 * (gt * gt);
  const float denom = sqrtf(v) / bc2sqrt + h.eps;
  p = p - step_size * (m / denom);
}

__global__ __launch_bounds__(kOptimThreads) void adam_apply_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                   float* __restrict__ v, int64_t n, const OptimState* __restrict__ st,
                                                                   OptimHyper h) {
  if (st->apply == 0) return;
  const float coef = st->coef, step_size = st->step_size, bc2sqrt = st->bc2sqrt_f32;
  const int64_t i = int64_t(blockIdx.x) * kOptimThreads + threadIdx.x;
  const int64_t nv = n >> 2;
  if (i < nv) {
    float4 pp = reinterpret_cast<float4*>(p)[i], mm = reinterpret_cast<float4*>(m)[i], vv = reinterpret_cast<float4*>(v)[i];
    const float4 gg = reinterpret_cast<const float4*>(g)[i];
    adam_element(pp.x, gg.x, mm.x, vv.x, coef, step_size, bc2sqrt, h);
    adam_element(pp.y, gg.y, mm.y, vv.y, coef, step_size, bc2sqrt, h);
    adam_element(pp.z, gg.z, mm.z, vv.z, coef, step_size, bc2sqrt, h);
    adam_element(pp.w, gg.w, mm.w, vv.w, coef, step_size, bc2sqrt, h);
    reinterpret_cast<float4*>(p)[i] = pp;
    reinterpret_cast<float4*>(m)[i] = mm;
    reinterpret_cast<float4*>(v)[i] = vv;
  } else if (i < nv + (n & 3)) {                               // the scalar tail: elements 4 nv .. n - 1
    const int64_t e = 4 * nv + (i - nv);
    float pe = p[e], me = m[e], ve = v[e];
    adam_element(pe, g[e], me, ve, coef, step_size, bc2sqrt, h);
    p[e] = pe;
    m[e] = me;
    v[e] = ve;
  }
}

}  // namespace wekws
