/*
 * wekws_hip.h -- C ABI of libwekws_hip.so, the MI355X (gfx950) implementation of the
 * WeKws keyword-spotting inference hot path.
 *
 * The reference has no C ABI of its own; the path sits behind two call boundaries
 * (paths relative to the reference tree):
 *   - Python   wekws/model/kws_model.py:65-76   KWSModel.forward(x, in_cache) -> (y, out_cache)
 *              wekws/model/kws_model.py:78-90   KWSModel.forward_softmax
 *   - C++      runtime/core/kws/keyword_spotting.h:26-55   wekws::KeywordSpotting::{ctor,Reset,Forward}
 *              runtime/core/frontend/fbank.h:138-198       wenet::Fbank::Compute
 * Every entry point below names the reference interface it replaces.  INTEGRATION.md shows
 * the ctypes / C++ stubs a reference maintainer would add to bind them.
 *
 * Conventions
 *   - plain C, no torch / STL types; all tensors are caller-owned DEVICE pointers (float32,
 *     contiguous unless a stride is given); the library owns only its device copy of the
 *     weights and scratch workspaces (one per model and calling stream, grown on demand).
 *   - every call is asynchronous on the hipStream_t passed as `void* stream` (NULL = the default stream of the
 *     object's device); no hidden synchronisation except when a scratch buffer has to grow (wekws_hip_reserve).
 *   - an object lives on the device it was created for; calls make that device current for their duration and
 *     restore the caller's current device before returning.
 *   - return value: 0 on success, a negative WEKWS_HIP_E* code on failure; the message is
 *     available from wekws_hip_last_error() (thread-local).  Nothing throws across the ABI.
 *   - a model is immutable after create: wekws_hip_forward is re-entrant across streams as
 *     long as each call has its own x / y / cache buffers.  Calls that need scratch memory
 *     (inputs longer than one LDS tile, the GRU) take it from the workspace of the stream they are
 *     issued on; growing a workspace synchronises that stream once.
 */
#ifndef WEKWS_HIP_H_
#define WEKWS_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WEKWS_HIP_ABI_VERSION 2 /* 2: wekws_hip_forward_status; failures of a stream surface on its next call */

/* frames one kernel launch keeps resident in LDS; longer inputs are processed as a sequence of
 * tiles that hand the causal left context over through the streaming cache */
#define WEKWS_HIP_TILE_FRAMES 112

enum wekws_hip_error {
  WEKWS_HIP_OK = 0,
  WEKWS_HIP_EINVAL = -1,      /* bad argument / unsupported configuration */
  WEKWS_HIP_ENOMEM = -2,      /* device allocation failed */
  WEKWS_HIP_EDEVICE = -3,     /* HIP runtime error (no device, launch failure ...) */
  WEKWS_HIP_ECAPACITY = -5,   /* a CTC keyword stream's prefix outgrew the capacity set at creation (never truncated) */
  WEKWS_HIP_EUNSUPPORTED = -4 /* valid reference config that this build has no kernel for.  Since ABI 2 no MODEL
                                 configuration returns it: shapes beyond the specialised kernels (more than 256 channels, kernel
                                 sizes above 8 / 5, GRU hidden sizes above 128 or pooled heads on a GRU, ...) run on the
                                 any-shape exact-f32 path (csrc/generic.hip.h; wekws_hip_effective_precision reports F32).
                                 That path is one launch per layer -- and for a GRU two launches per layer AND TIME STEP (2 T L
                                 launches per call: a correctness path; do not capture long GRU calls of such shapes into a graph).
                                 Left: fbank frame lengths outside 65 .. 512 samples. */
};

/* backbone.type of the reference model config (wekws/model/kws_model.py:126-170) */
enum wekws_hip_backbone {
  WEKWS_HIP_BACKBONE_DS_TCN = 0, /* type: tcn, ds: true   (wekws/model/tcn.py:91-119)  */
  WEKWS_HIP_BACKBONE_TCN = 1,    /* type: tcn, ds: false  (wekws/model/tcn.py:67-88)   */
  WEKWS_HIP_BACKBONE_MDTC = 2,   /* type: mdtc            (wekws/model/mdtc.py:201-276) */
  WEKWS_HIP_BACKBONE_GRU = 3,    /* type: gru             (wekws/model/kws_model.py:128-133) */
  WEKWS_HIP_BACKBONE_FSMN = 4    /* type: fsmn            (wekws/model/fsmn.py:394-495) */
};

/* classifier of the reference config (wekws/model/kws_model.py:175-199) */
enum wekws_hip_head {
  WEKWS_HIP_HEAD_LINEAR = 0,  /* LinearClassifier, per frame   (classifier.py:54-67) */
  WEKWS_HIP_HEAD_GLOBAL = 1,  /* GlobalClassifier, mean over T (classifier.py:19-28) */
  WEKWS_HIP_HEAD_LAST = 2,    /* LastClassifier, last frame    (classifier.py:31-40) */
  WEKWS_HIP_HEAD_IDENTITY = 3 /* classifier.type: identity     (kws_model.py:188-189) */
};

enum wekws_hip_activation {
  WEKWS_HIP_ACT_IDENTITY = 0,
  WEKWS_HIP_ACT_SIGMOID = 1, /* kws_model.py:196-199 */
  WEKWS_HIP_ACT_SOFTMAX = 2  /* the model *is* forward_softmax: what wekws/bin/export_onnx.py:46-48 exports for CTC
                                recipes (forward := forward_softmax before tracing).  Per-frame heads only; set by the
                                exported-file reader, never by a training config.  wekws_hip_forward then applies the
                                softmax whatever its `softmax` argument says. */
};

/* How the 1x1 / dense convolutions and Linear layers of the conv backbones are multiplied.  All modes read and
 * write float32 and accumulate in float32; F32 and F16X3 meet the 1e-4 posterior bar against the reference, F16 is the
 * opt-in reduced-precision mode of BASELINE.json's "fp16 weights + fp16 MFMA pointwise conv" configuration. */
enum wekws_hip_precision {
  WEKWS_HIP_PRECISION_DEFAULT = 0, /* library's choice: F16X3 */
  WEKWS_HIP_PRECISION_F32 = 1,     /* exact-f32 matrix instructions: each product rounded once like the reference's fp32
                                      math (conv backbones and GRU: MFMA kernels; FSMN, and every shape without a specialised
                                      kernel: the any-shape path of csrc/generic.hip.h -- v_mfma_f32_16x16x4_f32 for the
                                      matrix products, v_fma_f32 for the depthwise taps and the GRU cell) */
  WEKWS_HIP_PRECISION_F16X3 = 2,   /* operands split into fp16 hi + lo, three fp16 matrix products per term, with BLOCK
                                      FLOATING POINT: every weight matrix and every operand tile carries an exact
                                      power-of-two scale chosen from its magnitude, so the accuracy is fp32-level (~2^-22
                                      of the tile maximum) at ANY operand scale -- no overflow at 65504, no loss below
                                      fp16's normal range (csrc/conv_stack_f16.hip.h); ~5x the f32 matrix rate */
  WEKWS_HIP_PRECISION_F16 = 3      /* weights and activations rounded to fp16 where they enter a pointwise-conv / input
                                      Linear product, ONE matrix product per term, fp32 accumulate; depthwise taps,
                                      biases, residuals and the classifier stay fp32.  Posterior error vs the fp32
                                      reference ~1e-3 (tests state the bound).  Honoured by the 16-wave kernels
                                      (DS-TCN hidden 256 with a keyword head, MDTC hidden 64); every other shape runs
                                      F16X3, i.e. more accurate than asked. */
};

/*
 * Model descriptor = the reference's configs['model'] dict (kws_model.py:97-214) as plain ints.
 * The weights travel separately as ONE float32 blob with inference-time constants already
 * folded by the host packer (wekws_amd/pack.py): GlobalCMVN into the first Linear, every
 * eval-mode BatchNorm1d into the preceding conv, Dropout dropped.  Blob layout, in order
 * (row-major, all float32):
 *   preprocessing       Wpre[hdim][idim], bpre[hdim]
 *                       (preproc_relu = 0 encodes NoSubsampling / CMVN-only as a diagonal Wpre)
 *   DS_TCN  per block   wd[hdim][ksize], bd[hdim], Wp[hdim][hdim], bp[hdim]
 *   TCN     per block   W[hdim][hdim][ksize], b[hdim]
 *   MDTC    per block   wd[hdim][ksize], bd[hdim], W1[hdim][hdim], b1[hdim], W2[hdim][hdim], b2[hdim]
 *                       (block order: preprocessor, then stack 0 block 0 ... as mdtc.py:247-275)
 *   GRU     per layer   W_ih[3H][H], W_hh[3H][H], b_ih[3H], b_hh[3H]   (gate order r,z,n)
 *   head LINEAR         Wc[odim][hdim], bc[odim]
 *   head GLOBAL / LAST  W1[head_hidden][hdim], b1[head_hidden], W2[odim][head_hidden], b2[odim]
 *   head IDENTITY       (nothing; odim == hdim)
 *
 * FSMN (fsmn.py:394-495; always preprocessing none + identity head, fsmn_ctc.yaml:36-56) has no preprocessing /
 * head sections; its blob is
 *   in_linear1 W[aux0][idim], b[aux0]  (CMVN folded) ; in_linear2 W[hdim][aux0], b[hdim]
 *   per layer  Wproj[proj][hdim] (no bias), taps[proj][lorder + rorder], Waff[hdim][proj], baff[hdim]
 *              taps = [conv_left taps, +1 on the last (the block's identity path, fsmn.py:236-237) | conv_right taps]
 *   out_linear1 W[aux1][hdim], b[aux1] ; out_linear2 W[odim][aux1], b[odim]
 * with the descriptor slots read as: hdim = linear_dim, num_layers = fsmn layers, num_stack = proj_dim,
 * kernel_size = left_order, stack_size = right_order, aux[0] = input_affine_dim, aux[1] = output_affine_dim.
 * Memory blocks run with stride 1, as the reference builds them whatever left_stride / right_stride say
 * (fsmn.py:381-383).  The cache is 4-D: (B, proj_dim, left_order - 1 + right_order, layers), layer index innermost.
 */
typedef struct wekws_hip_desc {
  int32_t abi_version;  /* WEKWS_HIP_ABI_VERSION */
  int32_t backbone;     /* enum wekws_hip_backbone */
  int32_t idim;         /* input_dim  (feature dim, e.g. 40) */
  int32_t hdim;         /* hidden_dim (channels of the backbone) */
  int32_t odim;         /* output_dim (keywords / classes / tokens) */
  int32_t num_layers;   /* tcn / gru / fsmn: num_layers; mdtc: unused (0) */
  int32_t num_stack;    /* mdtc: num_stack; fsmn: proj_dim; else 0 */
  int32_t stack_size;   /* mdtc: stack_size; fsmn: right_order; else 0 */
  int32_t kernel_size;  /* tcn / mdtc conv kernel size; fsmn: left_order; gru: 0 */
  int32_t preproc_relu; /* 1: LinearSubsampling1 (Linear+ReLU, subsampling.py:39-61); 0: no ReLU */
  int32_t head;         /* enum wekws_hip_head */
  int32_t head_hidden;  /* GLOBAL / LAST: width of the MLP (64 in kws_model.py:181-186), else 0 */
  int32_t activation;   /* enum wekws_hip_activation */
  int32_t precision;    /* enum wekws_hip_precision */
  int32_t aux[2];       /* fsmn: input_affine_dim, output_affine_dim; every other backbone: must be 0 */
} wekws_hip_desc;

typedef struct wekws_hip_model wekws_hip_model;

/* Thread-local description of the last failure on the calling thread ("" if none). */
const char* wekws_hip_last_error(void);

/* ABI version the library was built with (== WEKWS_HIP_ABI_VERSION of its header). */
int wekws_hip_abi_version(void);

/* Number of float32 elements the weight blob for `desc` must hold; 0 if desc is invalid. */
size_t wekws_hip_blob_elems(const wekws_hip_desc* desc);

/*
 * Replaces: init_model(configs) + load_state_dict + .to(device)   (kws_model.py:97-214,
 * wekws/utils/checkpoint.py:23-36) and KeywordSpotting::KeywordSpotting(model_path)
 * (runtime/core/kws/keyword_spotting.cc:28-45).
 * host_blob: `n_elems` float32 on the HOST, layout above.  device: HIP device ordinal.
 */
int wekws_hip_create(const wekws_hip_desc* desc, const float* host_blob, size_t n_elems,
                     int device, wekws_hip_model** out);

void wekws_hip_destroy(wekws_hip_model* m);

/* Streaming-cache geometry, as the exporter publishes it in the ONNX metadata
 * (wekws/bin/export_onnx.py:55-77: cache_dim, cache_len).  Conv backbones: cache is
 * (B, cache_dim = hdim, cache_len = sum of paddings); GRU: (num_layers, B, hdim) and
 * cache_len = 0 (the reference cannot export GRU); FSMN: (B, cache_dim = proj_dim,
 * cache_len = left_order - 1 + right_order, num_layers) as export_onnx.py:57-60 shapes it. */
int wekws_hip_cache_dim(const wekws_hip_model* m);
int wekws_hip_cache_len(const wekws_hip_model* m);
/* float32 elements of the cache tensor for a batch of B streams */
size_t wekws_hip_cache_elems(const wekws_hip_model* m, int B);
/* float32 elements of y for (B, T): B*T*odim for per-frame heads, B*odim for GLOBAL/LAST */
size_t wekws_hip_output_elems(const wekws_hip_model* m, int B, int T);

/*
 * Kernel selection.  A model picks its kernels from its shape (DESIGN.md 3.1 "which kernel runs"); these options override
 * the choice -- for A/B measurements and for the tests that keep every kernel family parity-green.  They change speed,
 * never results beyond rounding (all families meet the same parity bar).  No environment variable is read anywhere.
 */
enum wekws_hip_option {
  WEKWS_HIP_OPT_W16 = 0,        /* DS-TCN hidden 256: 1 (default) the 16-wave kernel, 0 the generic 8-wave kernel */
  WEKWS_HIP_OPT_MDTC16 = 1,     /* MDTC hidden 64: 1 (default) the 16-wave kernel, 0 the generic 8-wave kernel */
  WEKWS_HIP_OPT_STREAM = 2,     /* chunks of <= 16 frames: 1 (default) the kernels with the LDS-resident cache, 0 the batch kernels */
  WEKWS_HIP_OPT_MM = 3,         /* DS-TCN hidden 256: the all-matrix-core kernel -- -1 (default) for CTC-sized heads only, 0 never, 1 whenever eligible */
  WEKWS_HIP_OPT_HEAD_SLICES = 4,/* workgroups sharing a CTC-sized last layer on small calls: -1 (default) automatic, 0 / 1 none, n exactly n */
  WEKWS_HIP_OPT_G16 = 5,        /* calls without an incoming cache: 1 (default) the register-resident kernels -- DS-TCN hidden 256: ds256_g16.hip.h (split fp16 / fp16) and ds256_g32.hip.h (precision F32), MDTC hidden 64: mdtc64_g4.hip.h --, 0 the LDS-tile kernels, 2 like 1 but one workgroup per utterance instead of persistent ones, 3 like 1 but calls WITH an incoming cache (later chunks of 17 .. 112 frames) keep the LDS-tile kernels instead of the register-resident kernels' context variants (measurement aids) */
  WEKWS_HIP_OPT_GRU_PIPE = 7,   /* GRU: 1 (default) the layer wavefront -- one launch, the stages of all layers running at the same time on different CUs (gru_pipe.hip.h) -- up to eight rounds of stream tiles per resident slot (B <= 128 x CUs / (2 x layers)), the layer-major kernels (gru_f16.hip.h) beyond; 2 the wavefront wherever it fits (at least 2 x layers CUs); 0 never; bit-identical results (csrc/route.h: select_gru_route) */
  WEKWS_HIP_OPT_ENVELOPE = 6    /* weights outside the split-fp16 envelope (wekws_hip_weight_spread_log2): 1 (default) run the exact-f32 kernels, 0 keep the split-fp16 kernels (to MEASURE where the envelope ends; accuracy is then not promised) */
};
int wekws_hip_set_option(wekws_hip_model* m, int option, int value);

/*
 * The arithmetic a model's calls REALLY run in (an enum wekws_hip_precision, never DEFAULT; negative error code for a NULL
 * model): desc.precision is a request, and not every backbone has a kernel for every mode -- F16 is reported when some call of
 * the model, under its current options, takes a kernel with a one-product variant (the DS-TCN h256 / h64 and MDTC h64 / h32
 * kernels of csrc/route.h; calls those kernels do not serve, and FSMN and every other shape, run F16X3: more accurate than
 * asked), a GRU without an fp16
 * kernel for its shape runs F32, every model on the any-shape path (csrc/generic.hip.h: shapes beyond the specialised
 * kernels; FSMN with precision F32 or with weights outside the split-fp16 envelope) runs F32 whatever was asked.  A caller
 * that needs exact-f32 reference rounding (a parity baseline) checks this instead of trusting the request.  Reflects the
 * kernel-selection options as they are set now.
 */
int wekws_hip_effective_precision(const wekws_hip_model* m);
/*
 * The envelope of the split-fp16 kernels.  Block floating point gives every weight matrix ONE power-of-two scale, so an
 * element keeps 22 significand bits only within 16 binades of the matrix maximum; a model whose matrices spread the
 * magnitudes of their rows (or of their K columns) over more than 2^WEKWS_HIP_F16X3_ENVELOPE_LOG2 would lose fp32-level
 * accuracy in the small rows (measured against the live reference: tests/golden/make_hetero_golden.py).  wekws_hip_create
 * measures the spread; a DEFAULT / F16X3 model beyond the envelope runs the exact-f32 kernels instead
 * (wekws_hip_effective_precision reports F32); an FSMN beyond it runs the any-shape exact-f32 path (csrc/generic.hip.h).
 *   wekws_hip_weight_spread_log2   the largest such spread of the model, in binades (-1 for a NULL model)
 */
#define WEKWS_HIP_F16X3_ENVELOPE_LOG2 20
float wekws_hip_weight_spread_log2(const wekws_hip_model* m);

/*
 * Scratch memory.  Inputs longer than one LDS tile (WEKWS_HIP_TILE_FRAMES frames; FSMN: 64) and every GRU call take
 * scratch from a grow-only buffer owned by (model, stream).  Growing it allocates, and frees the previous buffer behind
 * ONE synchronisation of that stream -- the only synchronisation the library ever performs on a caller's stream.  To keep
 * calls free of it (latency-critical loops; required before capturing a stream into a HIP graph, where a call that
 * would have to grow fails with WEKWS_HIP_EINVAL instead), size the buffer up front:
 *   wekws_hip_workspace_bytes  bytes a forward of exactly (B, T) needs (0: none).  NOT monotonic: a GRU chunk of <= 16
 *                              frames is spread over more workgroups and needs more scratch than a longer one
 *   wekws_hip_reserve          make the stream's buffer large enough for every call of at most B streams x at most T
 *                              frames now (the maximum of the above over the shapes where the launch geometry changes)
 *   wekws_hip_release          free the stream's buffer (e.g. before destroying the stream)
 */
size_t wekws_hip_workspace_bytes(const wekws_hip_model* m, int B, int T);
int wekws_hip_reserve(wekws_hip_model* m, int B, int T, void* stream);
int wekws_hip_release(wekws_hip_model* m, void* stream);
/*
 * Device-side health of the forwards issued on `stream` so far.  The GRU wavefront (WEKWS_HIP_OPT_GRU_PIPE) hands sequences
 * between workgroups inside one launch; every wait in it is bounded (~0.1 s), and a wait that gives up (a bug, or a device
 * whose other tenants keep the launch's later workgroups off the CUs for that long) ends the launch with garbage in the
 * outputs instead of hanging the GPU, and leaves a code in a word of pinned HOST memory owned by (model, stream).
 *   - the NEXT wekws_hip_forward on that (model, stream) reads the word (no synchronisation), launches nothing, clears it and
 *     returns WEKWS_HIP_EDEVICE: a caller that only ever calls forward -- the reference's scripts with the one-line import
 *     change -- cannot keep consuming garbage silently; wekws_hip_release returns it and wekws_hip_destroy leaves it in
 *     wekws_hip_last_error() if nobody asked before;
 *   - this call SYNCHRONISES the stream (for every model and stream, with or without such launches), then does the same
 *     check: WEKWS_HIP_EDEVICE (wekws_hip_last_error names the stage) if any forward since the last report gave up, else OK.
 * Nothing in the reference corresponds to it (ORT's Run is synchronous and throws, keyword_spotting.cc:77-79); call it
 * where results are consumed -- the C++ runtime does after every Forward (its one synchronisation), KWSModel.check() in Python.
 */
int wekws_hip_forward_status(wekws_hip_model* m, void* stream);

/*
 * Replaces: KWSModel.forward(x, in_cache) -> (y, out_cache)   (kws_model.py:65-76) and the body
 * of KeywordSpotting::Forward (keyword_spotting.cc:63-94, one ORT Run with the carried cache).
 *   x          (B, T, idim) device, contiguous
 *   in_cache   device, wekws_hip_cache_elems(m,B) floats, or NULL = the reference's empty-cache
 *              sentinel torch.zeros(0,0,0) (zero left context, tcn.py:49-52; zero h0 for GRU)
 *   y          device: (B, T, odim) for LINEAR / IDENTITY heads, (B, odim) for GLOBAL / LAST
 *   out_cache  device, same geometry as in_cache, or NULL if the caller does not need it;
 *              must not alias in_cache
 *   softmax    0: forward; 1: forward_softmax (softmax over the last axis, kws_model.py:89).
 *              Non-finite logits as torch.softmax has them: a class whose logit is -Inf (a masked
 *              class) gets exactly 0 and adds nothing to the other posteriors; a NaN or a +Inf
 *              anywhere in a row, or -Inf in every class, makes every posterior of that row NaN.
 *              Posteriors below float32's normal range (2^-126) may come out as 0.
 */
int wekws_hip_forward(wekws_hip_model* m, const float* x, int B, int T, const float* in_cache,
                      float* y, float* out_cache, int softmax, void* stream);

/* -------------------------------------------------------------------------------------------
 * The streaming step for many streams at once  --  KeyWordSpotter.forward's model call with its carried cache
 * (wekws/bin/stream_kws_ctc.py:486-487, `logits, self.in_cache = self.model(feats, self.in_cache)`), for any subset of the
 * streams of a pool in one call, every row with its own number of frames.  It sits between wekws_hip_stream_frontend_push, whose
 * `frames` it takes as they are, and wekws_hip_ctc_kws_step: a C caller has the whole pipeline, PCM in, detections out.
 *
 * The pool owns the streams' caches: (2, max_streams, wekws_hip_cache_elems(m, 1)) floats.  Every stream has two planes, one of
 * them live; a step reads the live plane and writes the other one, and the host flips the stream's parity bit in call order,
 * which is stream order.  No kernel reads and writes the same bytes (out_cache must not alias in_cache, as above), and a
 * stream that a call skips or leaves out keeps its plane.  All zeros is the empty-cache sentinel of every backbone.
 * A pool belongs to the model it was created for and must be destroyed before it.  Calls on one pool are serialised by a mutex and by
 * the caller's stream: use one stream per pool.
 * ------------------------------------------------------------------------------------------*/
typedef struct wekws_hip_stream_cache wekws_hip_stream_cache;
int wekws_hip_stream_cache_create(wekws_hip_model* m, int max_streams, wekws_hip_stream_cache** out);
void wekws_hip_stream_cache_destroy(wekws_hip_stream_cache* p);
/* ids: n stream ids, HOST int32 (NULL = every stream of the pool): those streams start from the empty-cache sentinel again.
 * A bad id returns WEKWS_HIP_EINVAL and resets nothing. */
int wekws_hip_stream_cache_reset(wekws_hip_stream_cache* p, const int32_t* ids, int n, void* stream);
/* One stream's live cache, in wekws_hip_forward's geometry for B = 1 (wekws_hip_cache_elems(m, 1) floats), to / from a device
 * buffer; ordered on `stream` like every other call. */
int wekws_hip_stream_cache_read(wekws_hip_stream_cache* p, int id, float* out, void* stream);
int wekws_hip_stream_cache_write(wekws_hip_stream_cache* p, int id, const float* in, void* stream);
/*
 * Row b of x (B, Tcap, idim) continues stream stream_ids[b] with its first frames[b] frames.
 *   stream_ids, frames  (B) HOST int32, as wekws_hip_stream_frontend_push takes and returns them; distinct ids, any subset of the
 *                       pool in any order.  frames[b] <= 0 (held, or nothing new): the row is skipped -- its stream's cache and its
 *                       row of y stay as they were
 *   y                   (B, Tcap, odim) device, or (B, odim) for GLOBAL / LAST heads: row b receives its frames[b] rows (its one row),
 *                       the rest is left as it was
 *   softmax             as for wekws_hip_forward, over the rows the call writes
 * A row's result is what wekws_hip_forward gives for that row alone with frames[b] frames and the stream's cache.
 * The whole call is checked on the host first: a bad or repeated id, frames[b] > Tcap, more rows than the pool has streams, or a
 * pool created for another model returns WEKWS_HIP_EINVAL (wekws_hip_last_error names the row), launches nothing and changes no
 * stream.  The per-row table travels to the device in stream order through a ring of pinned tables, so calls may be queued back to
 * back: the call does not synchronise, and does not allocate on the table-driven path below.  NOT inside a stream capture
 * (WEKWS_HIP_EINVAL): the table of a captured call would be rewritten by the next one.
 * Which kernels run (csrc/route.h: plan_streams):
 *   - DS-TCN hidden 256 with Tcap <= 16, and the FSMN kernel with Tcap within its tile: ONE launch that reads every row's frame
 *     count and cache planes from the table -- no copy of a cache besides the kernel's own read and write;
 *   - every other model, and longer rows: the rows are bucketed by frame count, and per bucket gathered out of the pool, run through
 *     wekws_hip_forward's kernels and scattered back, inside the library.  Its scratch grows on demand (one synchronisation), like a
 *     model's workspace.
 */
int wekws_hip_forward_streams(wekws_hip_model* m, wekws_hip_stream_cache* p, const float* x, int B, int Tcap,
                              const int32_t* stream_ids, const int32_t* frames, float* y, int softmax, void* stream);

/* -------------------------------------------------------------------------------------------
 * Fbank front-end  --  replaces wenet::Fbank::Compute (runtime/core/frontend/fbank.h:138-198)
 * with the framing rule of FeaturePipeline::AcceptWaveform (feature_pipeline.cc:30-47).
 * ------------------------------------------------------------------------------------------*/
enum wekws_hip_window {
  WEKWS_HIP_WINDOW_HAMMING = 0, /* the C++ runtime (fbank.h:90-96) */
  WEKWS_HIP_WINDOW_POVEY = 1    /* torchaudio.compliance.kaldi default (processor.py:196-202) */
};

typedef struct wekws_hip_fbank_cfg {
  int32_t num_bins;     /* 40 (or 80); 1..128, every triangular filter must cover an FFT bin (else EINVAL: the reference's
                           constructor CHECK-fails, fbank.h:81) */
  int32_t sample_rate;  /* 16000 */
  int32_t frame_length; /* samples, 400; 65..512 (the reference's 128- / 256- / 512-point FFT cases, fbank.h:43; else EUNSUPPORTED) */
  int32_t frame_shift;  /* samples, 160 */
  int32_t window;       /* enum wekws_hip_window */
  int32_t reserved[3];
} wekws_hip_fbank_cfg;

typedef struct wekws_hip_fbank wekws_hip_fbank;

int wekws_hip_fbank_create(const wekws_hip_fbank_cfg* cfg, int device, wekws_hip_fbank** out);
void wekws_hip_fbank_destroy(wekws_hip_fbank* f);
/* frames produced for nsamp samples: 1 + (nsamp - frame_length) / frame_shift, 0 if too short
 * (fbank.h:141-142) */
int wekws_hip_fbank_num_frames(const wekws_hip_fbank* f, int nsamp);
/*
 * pcm    (B, nsamp) device float32 in int16 scale (NOT divided by 32768; wav.h:98-102)
 * feats  (B, num_frames, num_bins) device float32
 */
int wekws_hip_fbank_compute(wekws_hip_fbank* f, const float* pcm, int B, int nsamp, float* feats,
                            void* stream);
/*
 * The same extractor on int16 PCM in device memory  --  the input of
 * FeaturePipeline::AcceptWaveform(const std::vector<int16_t>&) (feature_pipeline.cc:49-55): samples are widened to float
 * in registers (no /32768), so a caller that owns int16 audio uploads and reads 2 bytes per sample.  Bit-identical
 * features to wekws_hip_fbank_compute on the widened samples.
 *   pcm    (B, nsamp) device int16
 */
int wekws_hip_fbank_compute_i16(wekws_hip_fbank* f, const int16_t* pcm, int B, int nsamp, float* feats,
                                void* stream);

/*
 * The same extractor with DITHER  --  `dither` of kaldi.fbank / kaldi.mfcc as every training recipe of the reference sets it
 * (fbank_conf / mfcc_conf `dither: 1.0`, wekws/dataset/processor.py:134-203; the C++ stage: fbank.h:105,150-153): after the signal
 * is cut into frames and before the DC removal,  frame[i] += dither * N(0, 1),  an independent draw for every (frame, sample) of
 * the frame's frame_length samples, the signal in int16 scale.  The draws are made inside the kernel by a counter-based generator
 * (Philox4x32-10 + Box-Muller): the draw at (seed, row id, frame, sample) is a pure function of those four numbers, where row b of
 * the call has row id first_row + b  --  a data set cut into batches in any way gets the same noise per utterance, a repeated call
 * the same bits, and float32 PCM holding int16 values the bits of the int16 call.  One deviation from the reference: it draws
 * from torch's global CPU generator; that stream is not reproduced, the distribution and the place of the addition are.
 *   dither == 0            the plain call above, bit for bit (it IS that call)
 *   dither < 0, NaN, Inf   WEKWS_HIP_EINVAL, nothing is launched
 */
int wekws_hip_fbank_compute_dither(wekws_hip_fbank* f, const float* pcm, int B, int nsamp, float* feats, float dither,
                                   uint64_t seed, int64_t first_row, void* stream);
int wekws_hip_fbank_compute_dither_i16(wekws_hip_fbank* f, const int16_t* pcm, int B, int nsamp, float* feats, float dither,
                                       uint64_t seed, int64_t first_row, void* stream);
/*
 * The unit-variance normal field the two calls above scale by `dither` and add: out (B, nframes, frame_length) device float32,
 * out[b][t][i] the draw of (seed, first_row + b, frame t, sample i).  1 <= frame_length <= 512.  Runs on the current device.
 * The definition (generator, key, counter, sample mapping, uniforms, transform): csrc/philox.hip.h.
 */
int wekws_hip_dither_noise(uint64_t seed, int64_t first_row, int B, int nframes, int frame_length, float* out, void* stream);

/*
 * Context expansion + frame skip  --  replaces context_expansion / frame_skip of the data pipeline
 * (wekws/dataset/init_dataset.py:24-68, wekws/dataset/processor.py:267-311; fsmn_ctc.yaml:21-25 uses left 2,
 * right 2, skip 3: 80-d fbank -> the 400-d FSMN input at a third of the frame rate), fused into one gather:
 *   out[b][i][(lag + left) * F + f] = feats[b][max(i * skip + lag, 0)][f],   lag = -left .. right,
 *   i = 0 .. wekws_hip_splice_frames(T, right, skip) - 1
 * (the left margin replicates frame 0, the last `right` frames are dropped, then every skip-th frame is kept).
 */
/* ceil((T - right) / skip) for T >= right.  T < right (an utterance shorter than its right context): the reference's cut
 * feats_ctx[:, :T - right] is a negative slice that keeps 2 T - right frames (0 if that is <= 0), whose right-hand blocks are
 * torch.roll's wrap-around, frame (i * skip + lag) mod T -- reproduced bit for bit: ceil(max(2 T - right, 0) / skip). */
int wekws_hip_splice_frames(int T, int right, int skip);
/*
 * feats  (B, T, F) device float32
 * out    (B, wekws_hip_splice_frames(T, right, skip), (left + right + 1) * F) device float32
 * left >= 1 and left >= T: WEKWS_HIP_EINVAL -- the reference's left-margin loop (init_dataset.py:45-48) raises IndexError there.
 */
int wekws_hip_splice(const float* feats, int B, int T, int F, int left, int right, int skip, float* out,
                     void* stream);

/* -------------------------------------------------------------------------------------------
 * MFCC tail  --  what torchaudio.compliance.kaldi.mfcc does after its fbank call (the reference's MDTC recipes,
 * wekws/dataset/processor.py:160-169: num_ceps 80 of num_mel_bins 80):
 *   out = (logmel @ DCT) * lifter,  DCT = DCT-II 'ortho' (N x N) with column 0 := sqrt(1/N), first num_ceps columns;
 *   lifter_i = 1 + 0.5 Q sin(pi i / Q), Q = cepstral_lifter (22 in the reference's call; 0 disables it).
 * The log-mel rows come from wekws_hip_fbank_compute with WEKWS_HIP_WINDOW_POVEY.  torchaudio itself is not installable
 * here; parity is pinned against independent third-party implementations of the same algorithm (Hugging Face transformers'
 * numpy port of kaldi.fbank, scipy's DCT: tests/golden/kaldi_golden.npz) and a restatement of torchaudio's published code.
 *   logmel (rows, num_bins) device float32;  out (rows, num_ceps) device float32;  num_ceps <= num_bins <= 128
 * ------------------------------------------------------------------------------------------*/
int wekws_hip_dct_lifter(const float* logmel, int64_t rows, int num_bins, int num_ceps, float cepstral_lifter, float* out,
                         void* stream);

/*
 * Row softmax + top-k  --  the first beam prune of the CTC prefix beam search: `logits.softmax(2)` followed by
 * `probs.topk(score_beam_size)` per frame (wekws/bin/stream_kws_ctc.py:487-488, wekws/model/loss.py:236-238), fused so
 * that the (frames x vocabulary) posterior matrix is neither written nor copied to the host.
 *   logits (rows, K) device float32;  k in 1..8 (the reference uses 3)
 *   probs  (rows, k) device float32: the k largest softmax posteriors of each row, descending
 *   idx    (rows, k) device int32:   their column indices (equal values: lower index first; -1 if K < k)
 * Non-finite logits: a class masked with -Inf adds nothing to the denominator and follows the same rule for equal
 * values -- after the finite classes come the masked ones, probability 0, ascending index; they do not get -1, which is
 * kept for slots that no class fills.  A NaN logit is never selected: it makes every probability of its row NaN (as
 * torch.softmax does), the indices are those of the row's other classes in order, and slots left over -- fewer than k
 * classes that are not NaN -- hold (-1, 0) like the padding for K < k.  A +Inf logit ranks first and makes the row's
 * probabilities NaN; so does a row of -Inf alone (indices 0 .. k-1).  Indices are always in [0, K) or -1.
 */
int wekws_hip_softmax_topk(const float* logits, int64_t rows, int K, int k, float* probs, int32_t* idx,
                           void* stream);

/* -------------------------------------------------------------------------------------------
 * DET scoring  --  replaces the arithmetic of wekws/bin/compute_det.py:79-106 on the score lists that
 * wekws/bin/score.py:128-137 writes (one per utterance and keyword: the per-frame posteriors scores[b][0:len][k]),
 * so that an evaluation loop moves B*K maxima (+ B*n_thr counts) to the host instead of the (B, T, K) matrix.
 * Bit-exact: comparisons only.
 * ------------------------------------------------------------------------------------------*/
/*
 * Max pooling over time  --  compute_det.py:82-85 `score = max(score_list)` (a keyword utterance is a false reject at
 * threshold th iff max < th).
 *   scores     (B, T, K) device float32 (posteriors of wekws_hip_forward, per-frame heads)
 *   lengths    (B) device int32 valid frames per utterance (score.py:131 `logits[i][:feats_lengths[i]]`), clamped to
 *              [0, T]; NULL = T for every utterance
 *   max_out    (B, K) device float32; -inf for an empty utterance
 *   argmax_out (B, K) device int32 first frame that attains the maximum (list.index(max(list))), -1 if empty; or NULL
 */
int wekws_hip_score_maxpool(const float* scores, int B, int T, int K, const int32_t* lengths, float* max_out,
                            int32_t* argmax_out, void* stream);
/*
 * False-alarm counts of filler utterances  --  compute_det.py:88-96: per utterance and threshold,
 *   i = 0; while i < len: if score[i] >= th: n += 1; i += window_shift  else: i += 1
 *   keyword      column of `scores` (0 <= keyword < K)
 *   thresholds   (n_thr) device float64, the exact doubles the reference's `threshold += step` loop visits
 *   alarms       (B, n_thr) device int32
 * Scores are widened to double for the comparison, as Python does with the parsed floats.
 */
int wekws_hip_det_false_alarms(const float* scores, int B, int T, int K, int keyword, const int32_t* lengths,
                               const double* thresholds, int n_thr, int window_shift, int32_t* alarms, void* stream);
/*
 * The same scan on the scores AS THE REFERENCE'S TEXT FILE CARRIES THEM: score.py:134-135 writes '{:.6f}' and
 * compute_det.py parses that back, so every score is rounded to six decimals before it meets a threshold -- 0.4999997
 * is "0.500000" and counts as >= 0.5.  Use this one (and round the maxima of wekws_hip_score_maxpool the same way on the
 * host: rounding is monotonic, so max and rounding commute) to reproduce a stats file bit for bit; use the plain one for
 * the float32 posteriors themselves.
 */
int wekws_hip_det_false_alarms_text(const float* scores, int B, int T, int K, int keyword, const int32_t* lengths,
                                    const double* thresholds, int n_thr, int window_shift, int32_t* alarms, void* stream);

/* -------------------------------------------------------------------------------------------
 * CTC prefix beam search and keyword detection  --  the decode that turns a CTC head's posteriors into a keyword decision,
 * on the device, for many streams at once:
 *   offline    wekws/model/loss.py:206-312 ctc_prefix_beam_search + the per-utterance loop of wekws/bin/score_ctc.py:183-236
 *   streaming  wekws/bin/stream_kws_ctc.py KeyWordSpotter: the post-model part of forward (:488-514), decode_keywords,
 *              execute_detection, is_sublist, reset / reset_all (:516-530)
 * Every output is bit-identical to the reference given the same float32 posteriors (its arithmetic is Python floats: the
 * kernel computes in f64).  Two deliberate deviations: exact ties inside the first-beam top-k go lower
 * index first; a frame holding +-Inf fails its stream with WEKWS_HIP_EINVAL (NaN ranks above every number and is dropped
 * by the 0.05 filter, as in the reference).  A stream whose status is set is left untouched by later steps until
 * reset / reset_all.
 * ------------------------------------------------------------------------------------------*/
typedef struct wekws_hip_ctc_kws_desc {
  int32_t vocab;            /* V >= 1 */
  int32_t score_beam;       /* 1..8 (reference: 3) */
  int32_t path_beam;        /* 1..64 (reference: 20) */
  int32_t num_keywords;     /* >= 0 */
  const int32_t* keyword_tokens;   /* host: the keywords' token ids, concatenated in insertion order */
  const int32_t* keyword_offsets;  /* host: num_keywords + 1 offsets into keyword_tokens; every keyword non-empty */
  const int32_t* token_set;        /* host: the first-beam token set (KeyWordSpotter adds blank 0 itself: so must the
                                      caller), or NULL for none (loss.py's keywords_tokenset=None) */
  int32_t token_set_len;
  int32_t min_frames, max_frames, interval_frames;   /* streaming detection (reference: 5, 250, 50) */
  int32_t downsampling;     /* >= 1: frame t of a chunk is t * downsampling + total_frames */
  int32_t max_streams;      /* streaming slots, ids 0 .. max_streams - 1 */
  int32_t prefix_capacity;  /* streaming: longest prefix a stream may hold (ECAPACITY beyond) */
  int32_t device;
  double threshold;
} wekws_hip_ctc_kws_desc;

typedef struct wekws_hip_ctc_kws_result {
  int32_t status;   /* 0, or the stream's failure (WEKWS_HIP_EINVAL: +-Inf posterior or bad id / count; WEKWS_HIP_ECAPACITY) */
  int32_t valid;    /* streaming: 0 = the call gave the stream no frames (the reference's `{}`, nothing changed) */
  int32_t state;    /* streaming: 1 = activated (forward's result "state"); offline: 1 = a keyword was found */
  int32_t keyword;  /* keyword index of the last detection (activated or not), -1 = none */
  int32_t start, end;      /* its first / last node frame (the reference's start / end before * resolution) */
  double score;     /* hit_score: streaming, the stream's carried value after the call's last frame (reset to 1.0 only by
                       reset / activation / aging); offline, from 1.0 per utterance */
} wekws_hip_ctc_kws_result;

int wekws_hip_ctc_kws_create(const wekws_hip_ctc_kws_desc* desc, void** out);
void wekws_hip_ctc_kws_destroy(void* h);
/* Streaming step: row b of probs (B, T, V) device float32 continues stream stream_ids[b] with its first frames[b] frames
 * (0 .. T; 0 = the `{}` case).  stream_ids / frames (B) device int32 (frames NULL = T), distinct ids in one call, any
 * subset in any order; results (B) device.  Frame t of row b is stream time t * downsampling + total_frames. */
int wekws_hip_ctc_kws_step(void* h, const float* probs, int B, int T, const int32_t* stream_ids, const int32_t* frames,
                           wekws_hip_ctc_kws_result* results, void* stream);
/* Offline search: every row a fresh utterance of lengths[b] frames (NULL = T), decoded with the descriptor's beams and
 * token set, then score_ctc's detection.  beams: NULL, or (B) records of wekws_hip_ctc_kws_beam_bytes(h, T) bytes each
 * receiving the final beam.  Uses a workspace of the handle (grown on demand: synchronises `stream` once). */
int wekws_hip_ctc_kws_search(void* h, const float* probs, int B, int T, const int32_t* lengths,
                             wekws_hip_ctc_kws_result* results, void* beams, void* stream);
/* reset() (all = 0) or reset_all() (all = 1) of the n streams in ids (device int32); both clear a failed status. */
int wekws_hip_ctc_kws_reset(void* h, const int32_t* ids, int n, int all, void* stream);
/* Bytes of one beam record with prefix capacity `cap`:
 *   int32 count, pad | int32 len[PB rounded up to even] | f64 pb[PB] | f64 pnb[PB] | int32 token[PB][cap] |
 *   int32 frame[PB][cap] (+ 4 pad bytes if PB * cap is odd) | f64 prob[PB][cap];  rounded up to 16 bytes. */
size_t wekws_hip_ctc_kws_beam_bytes(void* h, int cap);
/* The beam of stream `id` (cur_hyps: prefix, pb, pnb and node token / frame / prob) into `out` (device, beam_bytes(h,
 * prefix_capacity)). */
int wekws_hip_ctc_kws_read_beam(void* h, int id, void* out, void* stream);
/* The stream's sticky status (0 or WEKWS_HIP_E*) into *status_out; synchronises `stream`. */
int wekws_hip_ctc_kws_status(void* h, int id, int32_t* status_out, void* stream);
/*
 * Keyword sets  --  KeyWordSpotter.set_keywords (wekws/bin/stream_kws_ctc.py:304-333) per STREAM instead of per object.  A set
 * is a keyword list, a first-beam token set (or none) and a threshold; the beams, min / max / interval frames, downsampling
 * and prefix capacity stay the handle's.  Set 0 is the descriptor's own and every stream starts in it: a program that never
 * registers a set sees no difference.  A result record's `keyword` is the index inside the stream's own set.
 * The calls are ordered against steps by `stream`, as reset is; a refused call (WEKWS_HIP_EINVAL: an unknown set, a bad or
 * repeated stream id, an empty keyword, a token outside the vocabulary, dropping a set in use) changes nothing and does no
 * device work.  Registering or dropping a set leaves every other stream's state and results alone.
 */
/* Register a keyword set on the handle; *set_out receives its id (>= 1; 0 is the descriptor's own set).
   Arguments as the descriptor's: token_set NULL = no first-beam set.  All arrays on the host. */
int wekws_hip_ctc_kws_add_set(void* h, const int32_t* keyword_tokens, const int32_t* keyword_offsets, int num_keywords,
                              const int32_t* token_set, int token_set_len, double threshold, int32_t* set_out, void* stream);
/* Drop a set no stream is assigned to (EINVAL otherwise, and for set 0); its id is reused, lowest first. */
int wekws_hip_ctc_kws_drop_set(void* h, int32_t set, void* stream);
/* Streams ids[i] (host, distinct) now use sets[i] (host) and are reset as by reset_all. */
int wekws_hip_ctc_kws_assign(void* h, const int32_t* ids, const int32_t* sets, int n, void* stream);
/* The set of stream `id` (host mirror, no device work); -1 for a bad id. */
int wekws_hip_ctc_kws_stream_set(void* h, int id);
/* wekws_hip_ctc_kws_search with a set per row (sets: host, B entries; NULL = set 0 for every row). */
int wekws_hip_ctc_kws_search_sets(void* h, const float* probs, int B, int T, const int32_t* lengths, const int32_t* sets,
                                  wekws_hip_ctc_kws_result* results, void* beams, void* stream);

/* -------------------------------------------------------------------------------------------
 * Streaming threshold detector  --  the detection of a max-pooling model (one sigmoid posterior per frame and keyword), for many
 * streams at once: the alarm scan of wekws/bin/compute_det.py:89-96 carried across chunks.  Per stream and keyword, each keyword
 * on its own, with a = the frame's index since the stream's reset:
 *   a frame FIRES iff a >= resume and (double)score >= thresholds[k] (a NaN never fires); then resume = a + window_shift
 *   best / best_frame: the running maximum since reset and its first frame (NaN ignored); -inf / -1 before any frame
 * For any split of a score sequence into chunks, empty ones included, the fired frames are those of one scan over the whole.
 * Scores are compared as float32 widened to double, like wekws_hip_det_false_alarms (not its `_text` variant).
 * ------------------------------------------------------------------------------------------*/
typedef struct wekws_hip_threshold_kws_slot {
  int32_t seen;        /* frames consumed since reset */
  int32_t resume;      /* first frame the scan looks at again */
  int32_t best_frame;  /* -1 before any frame */
  float best;          /* -inf before any frame */
} wekws_hip_threshold_kws_slot;

/* thresholds: (num_keywords) HOST float64;  window_shift >= 1;  stream ids 0 .. max_streams - 1 */
int wekws_hip_threshold_kws_create(int num_keywords, const double* thresholds, int window_shift, int max_streams, int device,
                                   void** out);
void wekws_hip_threshold_kws_destroy(void* h);
/* Dcap = ceil(Tcap / window_shift): the hits a chunk of Tcap frames can hold per keyword. */
int wekws_hip_threshold_kws_max_hits(void* h, int Tcap);
/*
 * probs       (B, Tcap, K) device float32; row b continues stream stream_ids[b] with its first frames[b] frames
 * stream_ids, frames  (B) device int32, as wekws_hip_ctc_kws_step takes them (frames NULL = Tcap); distinct ids, any subset
 * hit_frames  (B, K, Dcap) device int32: the fired frames of the chunk (indices since reset), ascending, -1 fill
 * hit_scores  (B, K, Dcap) device float32: their scores, 0 fill
 * best, best_frame  (B, K) device: the running maximum after the chunk
 * status      (B) device int32, or NULL: 0, or why the row was SKIPPED with its stream untouched (1: frames[b] outside
 *             0 .. Tcap; 2: id outside the pool; 3: the frame index would pass int32).  A skipped row's outputs hold the fills.
 * One launch, no synchronise.  No input value leads to an access outside the buffers as sized above.
 */
int wekws_hip_threshold_kws_step(void* h, const float* probs, int B, int Tcap, const int32_t* stream_ids, const int32_t* frames,
                                 int32_t* hit_frames, float* hit_scores, float* best, int32_t* best_frame, int32_t* status,
                                 void* stream);
/* The n streams in ids (device int32) start over: seen = resume = 0, no maximum.  Ids outside the pool are ignored. */
int wekws_hip_threshold_kws_reset(void* h, const int32_t* ids, int n, void* stream);
/* The state of (stream id, keyword) into *out (host); synchronises `stream`.  For tests. */
int wekws_hip_threshold_kws_state(void* h, int id, int keyword, wekws_hip_threshold_kws_slot* out, void* stream);

/* -------------------------------------------------------------------------------------------
 * Validation criterion  --  wekws/model/loss.py::criterion, forward only: what Executor.cv / Executor.test
 * (wekws/utils/executor.py:70-115) call after every forward, so that an evaluation loop moves two numbers per run to the
 * host instead of the (B, T, V) logits per batch.  Stateless; every pointer is a device pointer; no call synchronises or
 * allocates.  Deterministic: a row's outputs depend on that row alone, the batch totals are one fixed-order reduction (the
 * same inputs give the same bits on every run).  B, T, K, D, V >= 1.
 * ------------------------------------------------------------------------------------------*/
/*
 * max_pooling_loss (loss.py:26-88).
 *   scores      (B, T, K) device float32 posteriors;  target (B) device int32 (keyword column; < 0 or >= K: filler)
 *   lengths     (B) device int32, clamped to [0, T]; NULL = T.  (The reference fails unless lengths.max() == T; here the
 *               frames t >= lengths[b] are simply masked.)
 *   pooled      (B, K): column target[b]: max_t clamp(p, 1e-8, 1) with frames t >= len or t < min_duration counted as 0;
 *               every other column: min_t clamp(1 - p, 1e-8, 1) with frames t >= len counted as 1.  Bit-exact.
 *   loss_terms  (B, K) = -log(pooled);  loss (1) = sum(loss_terms) / B
 *   correct     (B) int32 0 / 1 by loss.py:74-85 (max over valid frames with masked frames 0, then over keywords, lower
 *               index on ties; > 0.5 and idx == target, or < 0.5 and target < 0);  num_correct (1) int32 = sum(correct)
 * A NaN in a valid frame makes that column's pooled value (and the loss) NaN and the utterance incorrect; a NaN in a masked
 * frame changes nothing.
 */
int wekws_hip_criterion_max_pooling(const float* scores, int B, int T, int K, const int32_t* target, const int32_t* lengths,
                                    int min_duration, float* pooled, float* loss_terms, int32_t* correct, float* loss,
                                    int32_t* num_correct, void* stream);
/*
 * cross_entropy + acc_frame (loss.py:167-180, :91-99).
 *   logits (B, D) device float32;  target (B) device int32
 *   loss_rows (B) = logsumexp(row) - row[target] (row max subtracted);  loss (1) = mean
 *   pred (B) int32 first arg-max;  correct (B) int32 = (pred == target);  num_correct (1) int32
 * A target outside [0, D) (torch raises; the device cannot without a synchronise) and a NaN logit make the row's loss NaN
 * and the row incorrect.
 */
int wekws_hip_criterion_ce(const float* logits, int B, int D, const int32_t* target, float* loss_rows, int32_t* pred,
                           int32_t* correct, float* loss, int32_t* num_correct, void* stream);
/*
 * ctc_loss without the accuracy (loss.py:154-162): log_softmax over V, F.ctc_loss(blank 0, reduction 'sum',
 * zero_infinity False) / B.
 *   logits (B, T, V) device float32, unnormalised;  targets (B, Lmax) device int32 labels in [1, V), row b's first
 *   target_lengths[b] entries (clamped to [0, Lmax]);  logit_lengths (B) clamped to [0, T]
 *   loss_rows (B): -log p(labels | logits); +Inf for a row no alignment fits (fewer frames than labels + adjacent repeats;
 *   no frames but labels); NaN for a row with a label outside [1, V) (torch raises).  loss (1) = sum(loss_rows) / B.
 *   probs: NULL, or (B, T, V) device float32 receiving the softmax of every frame t < logit_lengths[b] (the rest is left as
 *   it was): the posteriors that wekws_hip_ctc_kws_search decodes for the accuracy, from the same single read of the logits.
 *   workspace: wekws_hip_ctc_loss_workspace_bytes(B, T, Lmax) bytes of device scratch (per frame the log-probabilities of
 *   the blank and of the row's own labels; no (B, T, V) log-softmax is written).  Lmax <= 3000.
 */
size_t wekws_hip_ctc_loss_workspace_bytes(int B, int T, int Lmax);
int wekws_hip_ctc_loss(const float* logits, int B, int T, int V, const int32_t* targets, int Lmax, const int32_t* logit_lengths,
                       const int32_t* target_lengths, float* loss_rows, float* loss, float* probs, void* workspace,
                       size_t workspace_bytes, void* stream);
/*
 * acc_utterance after the decode (loss.py:119-132): the Levenshtein distance between entry 0 of each utterance's final beam
 * and its labels.
 *   beams   (B) records as wekws_hip_ctc_kws_search writes them for a handle of `path_beam` and T = `cap` frames
 *           (wekws_hip_ctc_kws_beam_bytes(h, cap) bytes each; a record with count 0 is the empty hypothesis)
 *   dist    (B) int32;  totals: NULL, or (2) int32 = {sum of target_lengths, sum of dist} over the rows with labels:
 *           the reference's accuracy is (totals[0] - totals[1]) * 100 / totals[0].   Lmax <= 3000.
 */
int wekws_hip_ctc_edit_distance(const void* beams, int path_beam, int cap, int B, const int32_t* targets, int Lmax,
                                const int32_t* target_lengths, int32_t* dist, int32_t* totals, void* stream);

/* -------------------------------------------------------------------------------------------
 * Streaming front end  --  the part of the streaming KeyWordSpotter that runs BEFORE the model, for many streams at once:
 *   wekws/bin/stream_kws_ctc.py:335-398 accept_wave: the samples left over from the last chunk (wave_remained), Kaldi fbank
 *   of (leftover + chunk), the last left + right feature frames for the context expansion (feature_remained) and the
 *   frame-skip phase (feats_ctx_offset), carried per stream.
 * int16 chunks of B streams go in, each row's new feature rows come out; a push is two launches (one without context and
 * skip), no sample or feature crosses to the host.  Per stream, with L = frame_length, S = frame_shift, l / r the context,
 * ds the skip and the state (rem, fr, off), a push of n samples:
 *   1. tot = rem + n < L r: every sample is kept and the row is HELD (the reference's None)            (:348-351)
 *   2. nf = 0 if tot < L else 1 + (tot - L) / S frames over [leftover | chunk]; rem' = tot - nf S       (:354-364)
 *      -- frame k of a stream is always samples [k S, k S + L) of its whole signal, and equals wekws_hip_fbank_compute_i16
 *      of those samples bit for bit (the kernels share the arithmetic)
 *   3. context: the reference asserts nf > r (EINVAL here); pad = l copies of the first new frame + the new frames on the
 *      stream's first processed chunk, else the remembered frames + the new ones; len(pad) - 2 r rows, row i = pad[i : i + l +
 *      r + 1]; fr' = the last l + r of the NEW frames only (after a chunk of fewer frames the next chunk's windows start
 *      late, as in the reference: reproduced, not judged)                                              (:366-390)
 *   4. skip: rows off, off + ds, ... of the k rows of step 3; off' = (off - k) mod ds                   (:391-397)
 * Context is either off (left = right = 0) or left == right >= 1: anything else is refused at creation (the reference raises
 * inside its window loop for left > right and silently drops right - left frames per chunk for left < right: INTEGRATION.md).
 * ------------------------------------------------------------------------------------------*/
typedef struct wekws_hip_stream_frontend_cfg {
  wekws_hip_fbank_cfg fbank; /* as for wekws_hip_fbank_create; frame_shift <= frame_length */
  int32_t left, right;       /* context: 0 / 0, or left == right >= 1 */
  int32_t skip;              /* >= 1 */
  int32_t max_streams;       /* stream ids 0 .. max_streams - 1 */
  int32_t max_chunk;         /* largest nmax of a push: sizes the fresh-frame workspace, so no push allocates or synchronises */
  int32_t device;
  int32_t reserved[2];
} wekws_hip_stream_frontend_cfg;

int wekws_hip_stream_frontend_create(const wekws_hip_stream_frontend_cfg* cfg, void** out);
/* The same front end delivering MFCC (the reference's MDTC recipes: wekws/dataset/processor.py:134-169): a fresh frame leaves the
 * fbank kernel as num_ceps cepstra -- DCT-II and cepstral lifter as wekws_hip_dct_lifter applies them, bit for bit, by the wave
 * that finished the frame; a push stays two launches -- and D below counts num_ceps where it says num_bins.  The handle is of the
 * kind _create returns: _push, _reset, _counts, _max_frames and _destroy take it; _plan does not depend on the feature width.
 * 0 < num_ceps <= cfg->fbank.num_bins <= 128 and cepstral_lifter >= 0 (0 disables it), else WEKWS_HIP_EINVAL. */
int wekws_hip_stream_frontend_create_mfcc(const wekws_hip_stream_frontend_cfg* cfg, int num_ceps, float cepstral_lifter, void** out);
void wekws_hip_stream_frontend_destroy(void* h);
/* The plan of one push for one stream, on the host alone (no device, no handle): counts_in = {rem, fr (-1 = none yet), off},
 * plan_out = {status, held, nf, rem_out, pad_first, fr_in, rows_ctx, rows_out, fr_out, off_out}.  Returns EINVAL for a
 * configuration or counts that no stream can have; a computed plan returns 0 and carries in status WEKWS_HIP_EINVAL where
 * the reference would trip its assertion (step 3).  This is the function push decides every row with. */
int wekws_hip_stream_frontend_plan(const wekws_hip_stream_frontend_cfg* cfg, const int32_t counts_in[3], int nsamp,
                                   int32_t plan_out[10]);
/* A row capacity Tcap that always suffices for chunks of up to nmax samples, whatever the streams hold. */
int wekws_hip_stream_frontend_max_frames(void* h, int nmax);
/*
 * pcm         (B, nmax) device int16, as the reference receives it; row b continues stream stream_ids[b] with its first
 *             nsamp[b] samples (0 .. nmax)
 * stream_ids  (B) HOST int32, distinct, any subset in any order;  nsamp (B) HOST int32
 * feats       (B, Tcap, D) device float32, D = num_bins without context, else (left + right + 1) * num_bins; row b receives
 *             its frames[b] rows, the rest of the row is left as it was
 * frames      (B) HOST int32 out: rows of each stream; -1 = held, 0 = the reference's empty result (no model call)
 * The whole call is planned on the host first: a bad or repeated stream id, nsamp[b] outside 0 .. nmax, nmax > max_chunk,
 * Tcap too small for a row, or a row where the reference would assert returns WEKWS_HIP_EINVAL, launches nothing and changes
 * no stream.  Pushes may be queued back to back on `stream` without a synchronise (the per-row plan travels in stream
 * order through a ring of pinned tables; not inside a stream capture).  Calls on one handle are serialised by a mutex and by
 * the caller's stream: use one stream per handle.
 */
int wekws_hip_stream_frontend_push(void* h, const int16_t* pcm, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp,
                                   float* feats, int Tcap, int32_t* frames, void* stream);
/* The n streams in ids (HOST int32) start over: no leftover, no remembered frames (the first-chunk pad comes back), phase 0. */
int wekws_hip_stream_frontend_reset(void* h, const int32_t* ids, int n);
/* counts_out = {rem, fr (-1 = none), off, rows delivered since creation / reset} of stream id. */
int wekws_hip_stream_frontend_counts(void* h, int id, int32_t counts_out[4]);

/* -------------------------------------------------------------------------------------------
 * Resampling  --  the `resample` step of the data pipeline (wekws/dataset/processor.py:83-103:
 * torchaudio.transforms.Resample(orig_freq, new_freq) with its defaults, sinc_interp_hann, lowpass_filter_width 6, rolloff
 * 0.99), for whole utterances and for chunks of many streams, on the device.  Parity is pinned to a float64 restatement of
 * torchaudio's published algorithm and to scipy.signal.upfirdn with the same taps.
 * With g = gcd(orig, new), o = orig / g, n = new / g, base = min(o, n) rolloff, width = ceil(lpw o / base), K = 2 width + o:
 *   t[i][m]    = clamp(((m - width) / o - i / n) base, -lpw, +lpw)          i = 0..n-1, m = 0..K-1   (float64)
 *   k[i][m]    = float32(sinc(pi t) cos^2(pi t / (2 lpw)) base / o)
 *   y[j n + i] = sum_m k[i][m] x[j o + m - width]                           x = 0 outside [0, L);  len(y) = ceil(n L / o)
 * Only the taps where the clamp is inactive are accumulated (the others are exactly 0 in float32), ascending in m, with fmaf
 * in float32.  Float input holding NaN / +-Inf is convolved over all K taps, as the reference does (0 NaN = NaN).  Equal
 * rates copy.  A pair whose table of live taps does not fit the kernel's LDS budget (64 KB) is refused at creation with
 * WEKWS_HIP_EUNSUPPORTED; {8000, 11025, 12000, 22050, 24000, 32000, 44100, 48000, 96000} -> 16000 and 16000 -> 8000 fit.
 * int16 output is rint (half to even) of the float32 sum, then saturation to [-32768, 32767].
 *
 * Streaming: a stream's output q is emitted by the first push after which every live tap of it lies on a received sample;
 * the concatenation of a stream's outputs, ended by a flush, equals the one-shot result of its whole signal bit for bit.
 * ------------------------------------------------------------------------------------------*/
enum wekws_hip_resample_out { WEKWS_HIP_RESAMPLE_OUT_F32 = 0, WEKWS_HIP_RESAMPLE_OUT_I16 = 1 };

typedef struct wekws_hip_resample_cfg {
  int32_t orig_freq, new_freq;   /* > 0 */
  int32_t lowpass_filter_width;  /* >= 1 (reference: 6) */
  int32_t out_dtype;             /* enum wekws_hip_resample_out */
  double rolloff;                /* 0 < rolloff <= 1 (reference: 0.99) */
  int32_t max_streams;           /* stream ids 0 .. max_streams - 1; 0 = one-shot only */
  int32_t max_chunk;             /* largest nmax of a push (>= 1 with streams) */
  int32_t device;
  int32_t reserved[3];
} wekws_hip_resample_cfg;

int wekws_hip_resample_create(const wekws_hip_resample_cfg* cfg, void** out);
void wekws_hip_resample_destroy(void* h);
/* ceil(new nsamp / orig) in 64 bits, on the host alone (no device, no handle); -1 for rates <= 0 or nsamp < 0. */
int64_t wekws_hip_resample_num_samples(int orig_freq, int new_freq, int64_t nsamp);
/*
 * One-shot.  pcm (B, nmax) device float32 (_compute) or int16 (_compute_i16); nsamp (B) HOST int32 valid samples per row, or
 * NULL = nmax;  out (B, mcap) device, float32 or int16 as the handle's out_dtype: row b receives its
 * wekws_hip_resample_num_samples(orig, new, nsamp[b]) samples and zeros behind them.  A row that yields more than mcap samples
 * returns WEKWS_HIP_EINVAL and launches nothing.  nmax, mcap <= 2^30 - 1.  Calls may be queued back to back on `stream` without
 * a synchronise (the row table travels through a ring of pinned tables, grown on demand: a call with more rows than any before
 * it allocates, so not inside a stream capture).  As for _push, calls on one handle are serialised by a mutex and by the
 * caller's stream: use one stream per handle, for _compute and _push alike.
 */
int wekws_hip_resample_compute(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, void* out, int mcap, void* stream);
int wekws_hip_resample_compute_i16(void* h, const int16_t* pcm, int B, int nmax, const int32_t* nsamp, void* out, int mcap,
                                   void* stream);
/*
 * Streaming.  pcm (B, nmax) device int16; row b continues stream stream_ids[b] with its first nsamp[b] samples (0 .. nmax);
 * stream_ids, nsamp (B) HOST int32, distinct ids, any subset in any order;  out (B, mcap) device as for _compute: row b
 * receives its counts[b] new samples and zeros behind them;  counts (B) HOST int32 out.  flush != 0 also emits every row's
 * tail, with zeros beyond the stream's last sample, up to ceil(new N / orig) in total, and ends the stream: a later push to it
 * is refused until it is reset.  The whole call is planned on the host first: a bad or repeated id, nsamp[b] outside 0 ..
 * nmax, nmax > max_chunk, a row that yields more than mcap samples or a push after a flush returns WEKWS_HIP_EINVAL, launches
 * nothing and changes no stream.  Pushes may be queued back to back on `stream` without a synchronise (the per-row plan
 * travels in stream order through a ring of pinned tables; not inside a stream capture).  Calls on one handle are serialised
 * by a mutex and by the caller's stream: use one stream per handle.
 */
int wekws_hip_resample_push(void* h, const int16_t* pcm, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp, int flush,
                            void* out, int mcap, int32_t* counts, void* stream);
/* A row capacity mcap that always suffices for chunks of up to nmax samples (with flush: the tail included). */
int wekws_hip_resample_max_out(void* h, int nmax, int flush);
/* The n streams in ids (HOST int32) start over: nothing received, nothing kept, not flushed. */
int wekws_hip_resample_reset(void* h, const int32_t* ids, int n);
/* counts_out = {samples received, samples emitted, samples kept on the device, flushed (0 / 1)} of stream id. */
int wekws_hip_resample_counts(void* h, int id, int64_t counts_out[4]);

/* -------------------------------------------------------------------------------------------
 * Rate bank  --  the resampler for rows and streams of DIFFERENT source rates in one launch.  The reference's `resample` step is
 * per utterance (wekws/dataset/processor.py:94-103: every sample carries its own sample_rate), so a batch may mix 8 kHz
 * telephony, 16 kHz devices and 44.1 / 48 kHz browser audio.  A bank holds up to WEKWS_HIP_RESAMPLE_BANK_MAX source rates
 * ("members", indexed in the order given) and one target rate; each row of a one-shot call names its member, each stream of a
 * streaming handle is assigned one.  A member is the resampler of its pair as defined above, with the bank's
 * lowpass_filter_width and rolloff; a member equal to the target copies.  A row's output equals the single-rate handle's for that
 * rate bit for bit.  One launch serves all rows: the (row, tile) list the workgroups walk is ordered by member and every
 * workgroup walks one contiguous span of it, reloading its tap table only where the member changes.
 * ------------------------------------------------------------------------------------------*/
#define WEKWS_HIP_RESAMPLE_BANK_MAX 16
/*
 * cfg as for wekws_hip_resample_create (max_streams == 0: one-shot only); orig_freqs (num_rates) HOST int32, the members;
 * cfg->orig_freq must equal orig_freqs[0].  WEKWS_HIP_EINVAL for an empty bank, more than WEKWS_HIP_RESAMPLE_BANK_MAX members, a
 * repeated rate or a rate <= 0; WEKWS_HIP_EUNSUPPORTED, with a message that names the member, for a member whose table does
 * not fit the LDS budget.  The LDS of a launch, the history capacity of a stream and max_out are the largest member's.
 */
int wekws_hip_resample_bank_create(const wekws_hip_resample_cfg* cfg, const int32_t* orig_freqs, int num_rates, void** out);
void wekws_hip_resample_bank_destroy(void* h);
/*
 * One-shot, as wekws_hip_resample_compute;  member_of_row (B) HOST int32 indices into the bank: row b receives its
 * wekws_hip_resample_num_samples(orig_freqs[member_of_row[b]], new, nsamp[b]) samples and zeros behind them.  Refusals as for
 * the single-rate call, plus a member index out of range: WEKWS_HIP_EINVAL, nothing launched.  The row table travels through
 * the same kind of ring of pinned tables.
 */
int wekws_hip_resample_bank_compute(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, const int32_t* member_of_row,
                                    void* out, int mcap, void* stream);
int wekws_hip_resample_bank_compute_i16(void* h, const int16_t* pcm, int B, int nmax, const int32_t* nsamp,
                                        const int32_t* member_of_row, void* out, int mcap, void* stream);
/*
 * The n streams in ids (HOST int32) use member `member` from now on and start over: nothing received, nothing kept, not
 * flushed.  A bad id or member is refused and changes no stream.  Streams start on member 0.
 */
int wekws_hip_resample_bank_set_rate(void* h, const int32_t* ids, int n, int member);
/* The source rate in Hz of stream id's member; WEKWS_HIP_EINVAL for a bad id. */
int wekws_hip_resample_bank_rate_of(void* h, int id);
/*
 * Streaming: the contracts of wekws_hip_resample_push, _max_out, _reset and _counts, every row planned with its stream's
 * member.  The whole call is planned on the host first, a refused call launches nothing and changes no stream, and a push is one
 * launch whatever the members of its rows.  nmax counts input samples at whatever rate; _max_out is the largest member's.
 */
int wekws_hip_resample_bank_push(void* h, const int16_t* pcm, int B, int nmax, const int32_t* stream_ids, const int32_t* nsamp,
                                 int flush, void* out, int mcap, int32_t* counts, void* stream);
int wekws_hip_resample_bank_max_out(void* h, int nmax, int flush);
int wekws_hip_resample_bank_reset(void* h, const int32_t* ids, int n);
int wekws_hip_resample_bank_counts(void* h, int id, int64_t counts_out[4]);

/* -------------------------------------------------------------------------------------------
 * Wire encodings  --  the rate bank fed the bytes a stream arrives in: G.711 telephony (one mu-law or A-law byte per sample),
 * unsigned 8-bit recordings, WebAudio float32, beside int16.  A member of a wire bank is a (rate, encoding) pair; the decode
 * happens in the resampler's fetch (no decode kernel, no decoded copy of the chunk in device memory) and every encoding decodes
 * one sample to one int16 value v, so the history of a stream, the arithmetic and the bit-for-bit contracts above stay as
 * they are: a wire row's output equals the _i16 call's on wekws_hip_wire_decode of that row, bit for bit.
 *
 *   S16    2 bytes, little endian   v = the value
 *   MULAW  1 byte c  (ITU-T G.711)  u = ~c & 0xFF;  t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4);
 *                                   v = (u & 0x80) ? 0x84 - t : t - 0x84                   0xFF, 0x7F -> 0;  0x80 -> 32124
 *   ALAW   1 byte c  (ITU-T G.711)  a = c ^ 0x55;  t = (a & 0x0F) << 4;  s = (a & 0x70) >> 4;  t += s ? 0x108 : 8;
 *                                   if (s > 1) t <<= s - 1;  v = (a & 0x80) ? t : -t        0xD5 -> 8;  0xAA -> 32256
 *   U8     1 byte c                 v = (c - 128) * 256
 *   F32    4 bytes, little endian,  v = rint(x * 32768.0f) (half to even; the product is exact), saturated to
 *          unit scale               [-32768, 32767] (+-Inf saturate), NaN -> 0: a wire row never takes the non-finite path
 * ------------------------------------------------------------------------------------------*/
enum wekws_hip_wire { WEKWS_HIP_WIRE_S16 = 0, WEKWS_HIP_WIRE_MULAW = 1, WEKWS_HIP_WIRE_ALAW = 2,
                      WEKWS_HIP_WIRE_U8 = 3, WEKWS_HIP_WIRE_F32 = 4 };
/* Bytes of one sample: 2, 1, 1, 1, 4;  0 for an unknown encoding. */
int wekws_hip_wire_sample_bytes(int encoding);
/* On the HOST: the n samples at src (host memory, any alignment) decoded to dst (n int16) by the definition above.
 * WEKWS_HIP_EINVAL for an unknown encoding, n < 0 or a NULL pointer with n > 0. */
int wekws_hip_wire_decode(int encoding, const void* src, int64_t n, int16_t* dst);
/*
 * wekws_hip_resample_bank_create with an encoding per member (encodings (num_rates) HOST int32, enum wekws_hip_wire).  The same
 * rate may appear with different encodings; a repeated (rate, encoding) pair and an unknown encoding are WEKWS_HIP_EINVAL, the
 * other refusals are _create's.  wekws_hip_resample_bank_create is this call with every encoding S16.  _destroy, _set_rate
 * (a member index), _rate_of, _max_out, _reset and _counts serve both kinds of handle.
 */
int wekws_hip_resample_bank_create_wire(const wekws_hip_resample_cfg* cfg, const int32_t* orig_freqs, const int32_t* encodings,
                                        int num_rates, void** out);
/*
 * wekws_hip_resample_bank_compute / _push on wire bytes.  pcm (B, row_bytes) device bytes: row b holds nsamp[b] samples in
 * its member's encoding from the row's first byte (_compute_wire: nsamp NULL = as many as row_bytes holds).  nsamp, max_chunk,
 * mcap and the counts keep counting SAMPLES.  Beside every refusal of the int16 calls (nsamp[b] is held against max_chunk, not
 * against an nmax): pcm not 4-byte aligned, row_bytes % 4 != 0, row_bytes > 2^30 - 4 or nsamp[b] * bytes > row_bytes are
 * WEKWS_HIP_EINVAL, planned on the host first: nothing is launched and no stream changes.  A push is one launch whatever the
 * members of its rows.  On a handle with members that are not S16, the int16 and float calls (_compute, _compute_i16, _push)
 * refuse a row of such a member with WEKWS_HIP_EINVAL; rows of S16 members behave as ever.
 */
int wekws_hip_resample_bank_compute_wire(void* h, const uint8_t* pcm, int B, int row_bytes, const int32_t* nsamp,
                                         const int32_t* member_of_row, void* out, int mcap, void* stream);
int wekws_hip_resample_bank_push_wire(void* h, const uint8_t* pcm, int B, int row_bytes, const int32_t* stream_ids,
                                      const int32_t* nsamp, int flush, void* out, int mcap, int32_t* counts, void* stream);
/* The encoding (enum wekws_hip_wire) of stream id's member; WEKWS_HIP_EINVAL for a bad id. */
int wekws_hip_resample_bank_encoding_of(void* h, int id);

/* -------------------------------------------------------------------------------------------
 * Augmentation  --  add_reverb, add_noise and spec_aug of the data pipeline (wekws/dataset/processor.py:374-392, 395-430,
 * 206-240) on the device, between the resampler and the front end.  What is drawn at random (whether a row is augmented, which
 * RIR or noise, where the noise starts, the SNR, the masks) is drawn by the caller and passed in HOST tables; every call checks
 * its tables on the host before anything is launched, and the tables reach the device in stream order without a
 * synchronisation, as wekws_hip_resample_compute's do (a ring of pinned tables grown on demand: not inside a stream capture
 * when a call is larger than any before it).  Calls on one handle are serialised by a mutex and by the caller's stream.
 *
 * Reverberation: y[n] = sum_{k=0..min(n, L-1)} h[k] x[n-k], h = rir / sqrt(sum rir^2) (the sum in double), n < the row's
 * length: signal.convolve(audio, h, 'full')[:len(audio)].  Computed as overlap-save convolution in float32 with the RIR in
 * uniform partitions: hop H = wekws_hip_reverb_hop() = 2048, transforms of 2H points, P = ceil(L / H) partitions, output block b
 * = the last H samples of the inverse transform of sum_{p=0..min(P-1, b)} X[b-p] Hf[p].  The partition spectra, transformed in
 * double on the host, stay on the device: sum over the RIRs of P (H + 1) complex float32 (8 bytes each).
 * ------------------------------------------------------------------------------------------*/
int wekws_hip_reverb_hop(void);
/* Without a device: out = {partitions of a rir_len-tap RIR, blocks of a row of nmax samples, bytes of scratch a call with B rows
 * of up to nmax samples needs, bytes of the RIR's spectra}.  WEKWS_HIP_EINVAL for rir_len < 1, B < 0, nmax < 0 or > 2^30 - 1. */
int wekws_hip_reverb_plan(int rir_len, int B, int nmax, int64_t out[4]);
/* Without a device: the check wekws_hip_reverb_apply makes of a call, against RIRs of these lengths. */
int wekws_hip_reverb_check(const int32_t* rir_lengths, int R, int B, int nmax, const int32_t* nsamp, const int32_t* rir_of_row);
/* rirs (R, max_len) HOST float32, lengths (R) HOST int32: RIR r is rirs[r][0 .. lengths[r]).  A length outside 1..max_len, a
 * NaN or an Inf among the taps, and an all-zero RIR (the reference divides by zero) are WEKWS_HIP_EINVAL. */
int wekws_hip_reverb_create(const float* rirs, const int32_t* lengths, int R, int max_len, int device, void** out);
void wekws_hip_reverb_destroy(void* h);
/* Bytes of scratch (the rows' input spectra) a call needs.  The handle owns the scratch and grows it on demand (a call larger
 * than any before it allocates: not inside a stream capture). */
size_t wekws_hip_reverb_workspace_bytes(void* h, int B, int nmax);
/* pcm, out (B, nmax) device float32 in any scale (the operation is linear);  nsamp (B) HOST int32 valid samples per row, NULL =
 * nmax;  rir_of_row (B) HOST int32: the row's RIR, -1 = the row is copied bit for bit.  Samples of out at or past nsamp[b] are
 * left as they were.  out == pcm, a length outside 0..nmax and an RIR index outside -1..R-1 are WEKWS_HIP_EINVAL and launch
 * nothing.  A row's result does not depend on the other rows, and two identical calls give identical bits.  A row with a NaN
 * or an Inf among its valid samples is NaN over its whole valid length (what the reference's FFT convolution gives); the
 * other rows are unaffected. */
int wekws_hip_reverb_apply(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, const int32_t* rir_of_row, float* out,
                           void* stream);
/* Noise at a drawn SNR.  noises (Rn, max_len) HOST float32 in int16 scale with a length each, as for the RIRs.  With
 *   v[n] = noise[(start + n) mod nlen]          (start + nsamp <= nlen where the noise is longer than the row: cut, not wrapped)
 *   audio_db = 10 log10(mean((pcm / pcm_scale)^2) + 1e-4),  noise_db = 10 log10(mean(v^2) + 1e-4)   (both sums in double)
 *   g = sqrt(10^((audio_db - noise_db - snr_db) / 10))      (in double on the device, rounded to float32)
 * out = pcm + pcm_scale g v, one fmaf a sample.  pcm_scale (> 0; rounded to float32) is 1 for samples in [-1, 1] and 32768 for
 * the int16-scale floats the front end takes.  noise_of_row -1 copies the row; start, snr_db (B) HOST; out may be pcm;
 * non-finite samples propagate as IEEE arithmetic has them.  start < 0, a start that runs a longer noise past its end, a
 * non-finite snr_db and the refusals of wekws_hip_reverb_apply are WEKWS_HIP_EINVAL and launch nothing. */
int wekws_hip_noise_create(const float* noises, const int32_t* lengths, int Rn, int max_len, int device, void** out);
void wekws_hip_noise_destroy(void* h);
/* Without a device: the check wekws_hip_noise_mix makes of a call, against noises of these lengths. */
int wekws_hip_noise_check(const int32_t* noise_lengths, int Rn, int B, int nmax, const int32_t* nsamp, const int32_t* noise_of_row,
                          const int32_t* start, const double* snr_db, double pcm_scale);
int wekws_hip_noise_mix(void* h, const float* pcm, int B, int nmax, const int32_t* nsamp, const int32_t* noise_of_row, const int32_t* start,
                        const double* snr_db, double pcm_scale, float* out, void* stream);
/* SpecAugment masks.  feats, out (B, T, F) device float32;  lengths (B) HOST int32 frames per row, NULL = T;  t_masks (B, nt, 2)
 * and f_masks (B, nf, 2) HOST int32 [start, end) pairs, already clipped as the reference clips them: 0 <= start <= end <= the
 * row's frames / F, else WEKWS_HIP_EINVAL.  Within a row's frames the frames of its time masks and the bins of its frequency
 * masks become 0; everything else, the frames past the row's length included, is copied.  out may be feats. */
int wekws_hip_spec_mask(const float* feats, int B, int T, int F, const int32_t* lengths, const int32_t* t_masks, int nt,
                        const int32_t* f_masks, int nf, float* out, void* stream);

/* -------------------------------------------------------------------------------------------
 * Global CMVN statistics  --  the accumulation of tools/compute_cmvn_stats.py (:26-72 per batch, :128-151 over the batches):
 * per bin the sum of the features ("mean_stat") and of their squares ("var_stat") over every valid frame, and the frame
 * count ("frame_num"), for features that are already on the device.  A handle keeps the running totals of its `dim` bins on
 * its device; calls on one handle are serialised by a mutex and by the caller's stream.
 *
 * Accumulation is in double from the first add ((double)x and its square are exact), where the reference adds in float32:
 * each statistic is within N 2^-53 sum|term| of the exact sum over the N frames added since the last reset.  The one
 * deviation from the reference: a sum that overflows float32 stays finite here.  Non-finite features propagate as IEEE
 * addition has them, per bin: a NaN gives NaN, +Inf alone +Inf, +Inf and -Inf together NaN in mean_stat and +Inf in var_stat.
 * The bits a call adds are a function of (feats, lengths, B, T, dim) alone: tiles of a fixed number of frames, their partial
 * sums folded in one fixed order, no floating-point atomics.
 * ------------------------------------------------------------------------------------------*/
/* dim outside 1..4096 is WEKWS_HIP_EINVAL (before any device work); no such device is WEKWS_HIP_EDEVICE. */
int wekws_hip_cmvn_stats_create(int dim, int device, void** out);
void wekws_hip_cmvn_stats_destroy(void* h);
/* Without a device: out = {frames a tile holds (from D alone), tiles of a call over (B, T, D), bytes of scratch the call needs:
 * 2 D doubles a tile, and for more than 64 tiles as much per 64 tiles}.
 * WEKWS_HIP_EINVAL for D outside 1..4096, a negative B or T, or more than 2^31 - 1 frames. */
int wekws_hip_cmvn_stats_plan(int B, int T, int D, int64_t out[3]);
/* feats (B, T, dim) device float32;  lengths (B) DEVICE int32 frames per row, NULL = T.  Frames at or past a row's length are
 * never read (a NaN in the padding does not reach the sums); a row whose length is outside 0..T adds nothing and is counted
 * as a bad row.  Asynchronous: two launches (three for more than 64 tiles), no synchronisation; the handle's scratch grows on
 * demand (a call larger than any before it allocates: not inside a stream capture).  A negative B or T, or more than 2^31 - 1
 * frames, is WEKWS_HIP_EINVAL. */
int wekws_hip_cmvn_stats_update(void* h, const float* feats, int B, int T, const int32_t* lengths, void* stream);
/* The totals and both counters start over (asynchronous). */
int wekws_hip_cmvn_stats_reset(void* h, void* stream);
/* mean_stat, var_stat (dim) HOST doubles; counts = {frame_num, bad_rows}.  The one call that synchronises (with `stream`). */
int wekws_hip_cmvn_stats_read(void* h, double* mean_stat, double* var_stat, int64_t counts[2], void* stream);

/* -------------------------------------------------------------------------------------------
 * The criterion's backward pass  --  the gradient of wekws/model/loss.py::criterion with respect to its input, what
 * torch's autograd gives for those statements, in closed form from what the forward kernels compute.  Conventions of the
 * forward calls: stateless, device pointers, no call synchronises or allocates, a row's gradient depends on that row alone,
 * every sum is a fixed-order reduction (the same inputs give the same bits on every run).  Every call writes
 *     g * upstream / divisor
 * into EVERY element of `grad` (so it may be uninitialised): g the gradient of the row's own loss (of the row's K loss terms
 * for max-pooling), exactly 0 in the frames t >= lengths[b];  upstream: a DEVICE pointer to one float, read by the kernel --
 * autograd's grad_output -- NULL = 1;  divisor: an int >= 1 -- B gives the gradient of the batch loss the reference returns,
 * 1 the rows' own gradients.  WEKWS_HIP_EINVAL (nothing launched) for a NULL pointer, a size < 1 or divisor < 1.
 * ------------------------------------------------------------------------------------------*/
/*
 * max_pooling_loss (loss.py:26-71) with respect to the posteriors; arguments as wekws_hip_criterion_max_pooling.
 *   column target[b]:  p_t = clamp(masked_t ? 0 : x_t, 1e-8, 1), masked_t = (t >= len or t < min_duration);  P = max_t p_t over
 *     ALL T frames, n = #{t : p_t == P} (masked frames count);  grad = -(1 / P) / n where p_t == P, the frame is not masked and
 *     1e-8 <= x_t <= 1 (the clamp's gate, inclusive: a winning 1.25 gets 0, a winning 1.0 gets -1), else 0
 *   other columns:  q_t = clamp(t >= len ? 1 : 1 - x_t, 1e-8, 1), Q = min_t q_t, n its ties over all T frames;
 *     grad = +(1 / Q) / n where q_t == Q, t < len and 1e-8 <= 1 - x_t <= 1, else 0
 * torch's full max() / min() split the gradient evenly among ties; so does this.  A NaN in an unmasked frame of a column
 * makes its pooled value NaN and the column's gradient all zeros (autograd routes the gradient to the NaN frames, where the
 * clamp's gate is false).  grad (B, T, K).
 */
int wekws_hip_criterion_max_pooling_grad(const float* scores, int B, int T, int K, const int32_t* target, const int32_t* lengths,
                                         int min_duration, const float* upstream, int divisor, float* grad /* (B,T,K) */,
                                         void* stream);
/*
 * cross_entropy (loss.py:178) with respect to the logits: grad (B, D) = softmax(row) - [d == target], from one read of the
 * row (running max, rescaled sum).  A target outside [0, D) or a NaN logit makes the whole row NaN (the forward's deviation).
 */
int wekws_hip_criterion_ce_grad(const float* logits, int B, int D, const int32_t* target, const float* upstream, int divisor,
                                float* grad /* (B,D) */, void* stream);
/*
 * ctc_loss (loss.py:154-162) with its gradient with respect to the logits; arguments and limits as wekws_hip_ctc_loss.
 *   loss_rows (B), loss (1): bit-identical to wekws_hip_ctc_loss on the same inputs (the same kernels).
 *   grad (B, T, V): on the frames t < len  softmax_t(v) - occ_t(v),  occ_t(v) = sum over the extended states s with
 *     l'_s == v of exp(alpha_t(s) + beta_t(s) - lp_t(v) + nll_b) -- alpha and beta in double, a class's states added in
 *     ascending order by one owner (no atomics);  0 on the frames t >= len;  NaN on the valid frames of a row no alignment
 *     fits (nll = +Inf, as torch) and of a row with a label outside [1, V) or a NaN logit;  all zeros for len == 0.
 *   workspace: wekws_hip_ctc_loss_grad_workspace_bytes(B, T, Lmax) bytes of device scratch, 8-byte aligned: the double alphas /
 *     occupancies of every frame (B T (2 Lmax + 1) doubles), the forward's log-probabilities, per frame the max and log-sum.
 * Five launches; the logits are read twice (the log-sum pass, the gradient pass), the gradient is written once.
 */
size_t wekws_hip_ctc_loss_grad_workspace_bytes(int B, int T, int Lmax);
int wekws_hip_ctc_loss_grad(const float* logits, int B, int T, int V, const int32_t* targets, int Lmax,
                            const int32_t* logit_lengths, const int32_t* target_lengths, const float* upstream, int divisor,
                            float* loss_rows, float* loss, float* grad /* (B,T,V) */, void* workspace, size_t workspace_bytes,
                            void* stream);

/* -------------------------------------------------------------------------------------------
 * The optimiser step  --  the last three statements of the reference's training step (wekws/utils/executor.py:58-60 with the
 * optimiser of wekws/bin/train.py:201):  grad_norm = clip_grad_norm_(parameters, clip);  if isfinite(grad_norm):
 * Adam.step()  --  over four flat float32 buffers of n elements each that the caller owns: params, grads, exp_avg,
 * exp_avg_sq.  The kernels take the four base pointers and n, never a table of per-tensor pointers.  Stateless calls, device
 * pointers, no call synchronises, allocates or reads a value on the host; every sum is a fixed-order reduction over tiles of a
 * fixed size (the bits of a step are a function of the buffers, the state block and the hyper-parameters alone; no
 * floating-point atomics).
 *
 * The state block: wekws_hip_optim_state_bytes() = 64 bytes of device memory, 16-byte aligned, zeroed by the caller before the
 * first step and from then on written by the calls alone:
 *     offset  0  int64   step         steps applied so far
 *             8  int64   skipped      steps not applied because the norm was not finite
 *            16  double  norm         the 2-norm of grads at the last call, from the double sum
 *            24  double  bc1          1 - beta1^step            (pow in double)
 *            32  double  bc2sqrt      sqrt(1 - beta2^step)
 *            40  float   coef         min(1, max_norm / (norm + 1e-6)) of the last call; exactly 1 for max_norm = +Inf
 *            44  float   norm_f32     float32(norm): what clip_grad_norm_ returns
 *            48  int32   apply        1: the last call stepped;  0: it wrote nothing but this block
 *            52  int32   finite       isfinite(norm_f32)
 *            56  float   step_size    float32(lr / bc1) of the last applied step
 *            60  float   bc2sqrt_f32  float32(bc2sqrt)
 *
 * A step, three launches (a fourth for more than 256 tiles):
 *     norm = sqrt(sum g^2), every square and every add in double;  finite = isfinite(float32(norm));
 *     apply = finite || !skip_nonfinite;  if apply: step += 1, else: skipped += 1 and nothing else is written;
 *     g~ = coef g + weight_decay p;  m' = beta1 m + (1 - beta1) g~;  v' = beta2 v + (1 - beta2) g~^2;
 *     p' = p - (lr / bc1) m' / (sqrt(v') / bc2sqrt + eps)
 * in float32, with correctly rounded sqrt and division: torch's single-tensor Adam.  grads is left as it was (the reference
 * scales it in place; here the coefficient is folded into the update).  The norm is summed in double: a gradient whose float32
 * sum of squares overflows while its norm is a finite float32 is clipped and stepped, where the reference skips the step.
 *
 * The hyper-parameters are doubles, as torch holds them: Adam forms 1 - beta2 in double before it rounds, and a float32
 * 0.999 would put that factor off by 1.3e-5 relative.
 * ------------------------------------------------------------------------------------------*/
/* Without a device: out = {floats a tile of the norm holds (a constant), tiles of n floats, bytes of workspace a call needs:
 * one double a tile and, for more than 256 tiles, one more per 256 tiles, rounded up to 16}.  WEKWS_HIP_EINVAL for n outside
 * 1 .. 2^28. */
int wekws_hip_optim_plan(int64_t n, int64_t out[3]);
size_t wekws_hip_optim_state_bytes(void);
/* WEKWS_HIP_EINVAL, before any launch, for: a NULL pointer; n outside 1 .. 2^28; a pointer that is not 16-byte aligned; two of
 * the four buffers overlapping; lr, eps or weight_decay negative, NaN or infinite; a beta outside [0, 1); max_norm <= 0 or NaN
 * (+Inf: no clipping); a workspace smaller than wekws_hip_optim_plan says.  skip_nonfinite 0: the step is applied whatever the
 * norm (plain Adam.step()). */
int wekws_hip_clip_adam_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                             void* state /* device, zero-initialised by the caller before the first step */, double lr, double beta1,
                             double beta2, double eps, double weight_decay, double max_norm /* +Inf: no clipping */,
                             int skip_nonfinite, void* workspace, size_t workspace_bytes, void* stream);
/* *norm_out (device) = float32 of the same norm, by the same two (three) launches: the bits of `norm_f32` above. */
int wekws_hip_grad_norm(const float* grads, int64_t n, float* norm_out /* device */, void* workspace, size_t workspace_bytes,
                        void* stream);

/* -------------------------------------------------------------------------------------------
 * The trainable FSMN memory block  --  FSMNBlock.forward with an empty cache (wekws/model/fsmn.py:214-253) and its autograd, as a
 * causal sparse FIR per channel.  x, y, grad_y, grad_x: (B, T, D) float32, contiguous;  w_left: (D, lorder), the memory of
 * conv_left.weight (D, 1, lorder, 1);  w_right: (D, rorder), the same for conv_right.weight.  With R = rorder * rstride and
 * x[b, n, d] = 0 for n < 0:
 *     y[b,t,d]   = x[b,t-R,d] + sum_i w_left[d,i] x[b, t-R-(lorder-1-i) lstride, d] + sum_j w_right[d,j] x[b, t-R+(j+1) rstride, d]
 *     grad_x     = the same taps run the other way over grad_y (terms past the row's end do not exist)
 *     grad_w_*   = the sums over b and t of grad_y times the frame of x the tap reads
 * Products are exact float32 fmaf in one order: skip term, left taps with i ascending, right taps with j ascending; the zeros
 * before frame 0 are arithmetic zeros (an Inf or NaN tap makes the first frames NaN, as the reference's padding does).  A row's
 * y and grad_x depend on that row alone.  The tap gradients are summed in double, per tile of 128 frames of a row in ascending
 * frame order, then over the tiles in a fixed order, and rounded to float32 once: their bits are a function of the inputs and
 * the shape.  Stateless calls, device pointers, no floating-point atomics; no call synchronises, allocates or reads on the host;
 * every element of every output is written.  16-byte accesses where D % 4 == 0 and the tensors' bases are 16-byte aligned,
 * scalar accesses with the same bits otherwise.
 *
 * Limits (WEKWS_HIP_EINVAL, before any launch): B, T, D >= 1;  lorder, rorder >= 1;  strides >= 1;  lorder + rorder <= 32;
 * a window R + (lorder-1) lstride + 1 of at most 256 frames.  forward: one launch;  backward: at most three.
 * ------------------------------------------------------------------------------------------*/
/* Without a device: bytes of workspace a backward call that wants the tap gradients needs: one double per tile of 128 frames of a
 * row, tap and channel, rounded up to 16.  0 on bad arguments. */
size_t wekws_hip_fsmn_memory_workspace_bytes(int B, int T, int D, int lorder, int rorder);
int wekws_hip_fsmn_memory_forward(const float* x, int B, int T, int D, const float* w_left, int lorder, int lstride,
                                  const float* w_right, int rorder, int rstride, float* y, void* stream);
/* grad_x NULL: not wanted.  grad_w_left and grad_w_right: both or neither (NULL: not wanted; then workspace may be NULL).  Also
 * WEKWS_HIP_EINVAL for: one tap gradient without the other; a workspace that is NULL, not 16-byte aligned or smaller than
 * wekws_hip_fsmn_memory_workspace_bytes says, when the tap gradients are wanted. */
int wekws_hip_fsmn_memory_backward(const float* x, const float* grad_y, int B, int T, int D, const float* w_left, int lorder,
                                   int lstride, const float* w_right, int rorder, int rstride, float* grad_x /* NULL: not wanted */,
                                   float* grad_w_left, float* grad_w_right, void* workspace, size_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------
 * The trainable depthwise Conv1d  --  nn.Conv1d(C, C, K, dilation=d, groups=C) behind F.pad(x, (left_pad, 0)): DsCnnBlock.cnn[0]
 * (wekws/model/tcn.py:102-107) and DSDilatedConv1d.conv (wekws/model/mdtc.py:37-46), and its autograd.  x, grad_x: (B, C, Tin)
 * float32, contiguous, time innermost;  y, grad_y: (B, C, Tout), Tout = Tin + left_pad - (K-1) d;  w: (C, K), the memory of
 * conv.weight (C, 1, K);  bias: (C) or NULL.  left_pad = P counts zeros the kernels supply in front of every row in place of
 * F.pad.  With xp[b, c, n] = 0 for n < 0:
 *     y[b,c,t]      = bias[c] + sum_k w[c,k] xp[b,c, t + k d - P]
 *     grad_x[b,c,n] = sum_k w[c,k] grad_y[b,c, n + P - k d]      (terms with an index outside [0, Tout) do not exist)
 *     grad_w[c,k]   = sum_{b,t} grad_y[b,c,t] xp[b,c, t + k d - P]          grad_bias[c] = sum_{b,t} grad_y[b,c,t]
 * y starts from the bias (+0 without one) and adds the taps with k ascending by exact float32 fmaf; grad_x adds the same taps,
 * k ascending.  The padding's zeros are arithmetic zeros in y and grad_w (an Inf or NaN tap makes the first P frames NaN, as the
 * reference's padding does).  A row's y and grad_x depend on that row alone.  grad_w and grad_bias are summed in double, per
 * tile of 128 frames of a (b, c) row in a fixed order, then over the tiles in a fixed order, and rounded to float32 once: their
 * bits are a function of the inputs and the shape.  Stateless calls, device pointers, no floating-point atomics; no call
 * synchronises, allocates or reads on the host; every element of every output is written.  16-byte accesses where Tin % 4 == 0,
 * Tout % 4 == 0 and the tensors' bases are 16-byte aligned, scalar accesses with the same bits otherwise.
 *
 * Limits (WEKWS_HIP_EINVAL, before any launch): B, C, Tin >= 1;  1 <= K <= 32;  d >= 1;  a window (K-1) d + 1 of at most 256
 * frames;  0 <= left_pad <= (K-1) d;  Tout >= 1.  forward: one launch;  backward: at most three.
 * ------------------------------------------------------------------------------------------*/
/* Without a device: bytes of workspace a backward call that wants grad_w or grad_bias needs: one double per batch row, tile of
 * 128 output frames, channel and tap (and one for the bias), rounded up to 16.  0 on bad arguments. */
size_t wekws_hip_depthwise_conv1d_workspace_bytes(int B, int C, int Tin, int K, int dilation, int left_pad);
int wekws_hip_depthwise_conv1d_forward(const float* x, int B, int C, int Tin, const float* w, const float* bias /* NULL: none */,
                                       int K, int dilation, int left_pad, float* y, void* stream);
/* grad_x, grad_w, grad_bias: each NULL when not wanted; its work is dropped.  workspace may be NULL when neither grad_w nor
 * grad_bias is wanted; otherwise also WEKWS_HIP_EINVAL for a workspace that is NULL, not 16-byte aligned or smaller than
 * wekws_hip_depthwise_conv1d_workspace_bytes says. */
int wekws_hip_depthwise_conv1d_backward(const float* x, const float* grad_y, int B, int C, int Tin, const float* w, int K, int dilation,
                                        int left_pad, float* grad_x, float* grad_w, float* grad_bias, void* workspace,
                                        size_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------
 * The trainable BatchNorm1d with the ReLU and the residual add that follow it  --  DsCnnBlock.cnn[1:3] / [4:6] (wekws/model/tcn.py),
 * DSDilatedConv1d.bn, TCNBlock.bn1 / relu1 and TCNBlock.bn2 + inputs + relu2 (wekws/model/mdtc.py), and their autograd.  x, y,
 * residual, grad_*: (B, C, T) float32, contiguous, time innermost (a (B, C) input is T = 1);  weight, bias, running_mean,
 * running_var, save_mean, save_invstd, grad_weight, grad_bias: (C);  num_batches_tracked: one int64.  N = B T.  Per channel:
 *     batch_stats != 0:  mean = sum x / N,  var = sum (x - mean)^2 / N (biased),  invstd = 1 / sqrt(var + eps)
 *     batch_stats == 0:  mean = running_mean,  invstd = 1 / sqrt(running_var + eps)
 *     z = (x - mean) invstd weight + bias (+ residual)          y = relu ? max(z, 0) : z   (a NaN stays a NaN)
 *     batch_stats and running buffers:  num_batches_tracked += 1;  f = momentum, or 1 / num_batches_tracked when momentum < 0;
 *         running_mean <- (1 - f) running_mean + f mean;  running_var <- (1 - f) running_var + f var N / (N - 1)
 *     backward, g' = grad_y where the ReLU passed (not y <= 0), all of it without ReLU:
 *         grad_residual = g'      grad_bias = sum g'      grad_weight = invstd sum g' (x - mean)
 *         grad_x = weight invstd (g' - grad_bias / N - (x - mean) invstd^2 sum g' (x - mean) / N)      (batch_stats)
 *         grad_x = weight invstd g'                                                                      (otherwise)
 * The sums are double sums over tiles of 128 frames of a (b, c) row in a fixed order, then over the tiles in a fixed order; the
 * statistics' sums are taken of x minus the channel's first element.  Every statistic, running value and parameter gradient is
 * computed in double and rounded to float32 once, so their bits are a function of the inputs and the shape; the float32
 * operation order of y and grad_x is stated in csrc/batchnorm.hip.h.  save_mean and save_invstd are written in both modes and are
 * what backward reads.  Stateless calls, device pointers, no floating-point atomics; no call synchronises, allocates or reads on
 * the host (num_batches_tracked is read and written on the device); every element of every output is written.  16-byte accesses
 * where T % 4 == 0 and the tensors' bases are 16-byte aligned, scalar accesses with the same bits otherwise.
 *
 * Limits (WEKWS_HIP_EINVAL, before any launch): B, C, T >= 1;  batch_stats with B T < 2;  batch_stats == 0 without running
 * buffers;  one running buffer without the other;  momentum < 0 with running buffers and no num_batches_tracked;  eps <= 0;
 * momentum > 1;  ceil(B C / 8) ceil(T / 128) workgroups above 2^31 - 1.  forward: three launches with batch statistics, one
 * without;  backward: at most three.
 * ------------------------------------------------------------------------------------------*/
/* Without a device: bytes of workspace a call needs: two doubles per batch row, tile of 128 frames and channel, two floats per
 * channel and 16 bytes, each part rounded up to 16.  0 on bad arguments. */
size_t wekws_hip_batchnorm_workspace_bytes(int B, int C, int T);
/* The workspace may be NULL when batch_stats == 0; otherwise also WEKWS_HIP_EINVAL for a workspace that is NULL, not 16-byte
 * aligned or smaller than wekws_hip_batchnorm_workspace_bytes says. */
int wekws_hip_batchnorm_forward(const float* x, const float* residual /* NULL: none */, int B, int C, int T,
                                const float* weight /* NULL: 1 */, const float* bias /* NULL: 0 */, float* running_mean /* NULL: none */,
                                float* running_var /* NULL: none */, int64_t* num_batches_tracked /* NULL: none */, int batch_stats,
                                double momentum /* < 0: cumulative */, double eps, int relu, float* y, float* save_mean,
                                float* save_invstd, void* workspace, size_t workspace_bytes, void* stream);
/* y: needed iff relu (WEKWS_HIP_EINVAL without it).  grad_x, grad_residual, grad_weight, grad_bias: each NULL when not wanted;
 * its work is dropped.  The workspace is needed for grad_weight, grad_bias and for grad_x under batch_stats. */
int wekws_hip_batchnorm_backward(const float* x, const float* y, const float* grad_y, int B, int C, int T,
                                 const float* weight /* NULL: 1 */, const float* save_mean, const float* save_invstd, int batch_stats,
                                 int relu, float* grad_x, float* grad_residual, float* grad_weight, float* grad_bias, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------
 * The trainable GRU's recurrent scan  --  the time loop of one layer of torch.nn.GRU(batch_first=True), the reference's gru
 * backbone (wekws/model/kws_model.py:128-133), and its backward through time.  PyTorch's gate order r, z, n; H the hidden size.
 * gi, grad_gi, grad_gh: (B, T, 3H) float32, contiguous;  y, grad_y: (B, T, H);  h0, hn, grad_hn, grad_h0: (B, H);  w_hh: (3H, H),
 * the parameter weight_hh_l* as it is;  b_hh: (3H);  reserve: (B, T, 4H), r, z, n and q of every step.  gi = W_ih x + b_ih is the
 * caller's GEMM.  With s the logistic function:
 *     gh = W_hh h[t-1] + b_hh      r = s(gi_r + gh_r)   z = s(gi_z + gh_z)   q = gh_n   n = tanh(gi_n + r q)
 *     y[t] = h[t] = (1 - z) n + z h[t-1]          hn = h[T-1]
 *     backward, t = T-1 .. 0, dh = grad_y[t] + carry (carry starts at grad_hn):
 *         dn = dh (1 - z)(1 - n^2)    dz = dh (h[t-1] - n) z (1 - z)    dr = dn q r (1 - r)
 *         grad_gi[t] = (dr, dz, dn)   grad_gh[t] = (dr, dz, dn r)       carry = dh z + W_hh^T grad_gh[t]
 *     grad_h0 = the last carry
 * The weight, bias and input gradients are the caller's GEMMs and column sums: dW_ih = grad_gi^T x, dW_hh = grad_gh^T h_prev,
 * dx = grad_gi W_ih, db_ih = sum grad_gi, db_hh = sum grad_gh.  Products are exact float32 on the matrix cores, added over
 * k ascending; the float32 operation order of the cell and of its gradient is stated in csrc/gru_train.hip.h; s and tanh saturate
 * without a NaN and a NaN goes through.  A row's results depend on that row alone: the same bits in any batch position, alone,
 * and on any run.  Stateless calls, device pointers, no floating-point atomics; no call synchronises, allocates or reads on the
 * host; every element of every output is written.  Each call is one launch: a workgroup owns 16 batch rows for all T steps.
 *
 * Limits (WEKWS_HIP_EINVAL, before any launch): B, T >= 1;  H % 16 == 0;  16 <= H <= 128;  every tensor 16-byte aligned;  the
 * pointers a call needs (forward: gi, w_hh, y, hn;  backward: y, reserve, w_hh, grad_gi, grad_gh).
 * ------------------------------------------------------------------------------------------*/
/* Without a device: bytes of the reserve a forward call leaves for the backward, B T 4H floats.  0 on bad arguments. */
size_t wekws_hip_gru_scan_reserve_bytes(int B, int T, int H);
int wekws_hip_gru_scan_forward(const float* gi, const float* w_hh, const float* b_hh /* NULL: none */, const float* h0 /* NULL: zeros */,
                               int B, int T, int H, float* y, float* hn, float* reserve /* NULL: not wanted */, void* stream);
/* y and reserve: what the forward call wrote;  h0: what it was given.  grad_y and grad_hn: each NULL for zeros.  grad_h0 NULL:
 * not wanted. */
int wekws_hip_gru_scan_backward(const float* grad_y, const float* grad_hn, const float* y, const float* h0, const float* reserve,
                                const float* w_hh, int B, int T, int H, float* grad_gi, float* grad_gh, float* grad_h0, void* stream);

/* -------------------------------------------------------------------------------------------
 * The Linear layers' weight and bias gradients  --  for y = x W^T + b with x (R, I) and the upstream gradient g (R, O), float32,
 * row-major and contiguous (R = B T rows, tens of thousands; O and I a few hundred):
 *     grad_w (O, I) = g^T x          grad_bias (O) = the column sums of g
 * as a split-K product whose arithmetic is stated, so the bits are a function of the inputs and the shape:
 *     chains   the R axis is cut into chains of 512 rows counted from row 0; per chain the float32 fmaf chain over its rows
 *              ascending from +0, on the matrix cores (exact float32 products); the boundaries depend on R alone
 *     slices   a slice is a run of consecutive chains, one workgroup's work for one 64 x 64 tile of grad_w: its chains are added
 *              in double, ascending, and the double partial goes to the workspace
 *     fold     the slices' doubles are added in ascending order and rounded to float32 once
 *     bias     the same on a column of ones: per chain a float32 ascending sum, then the same doubles
 * The number of slices depends on (R, O, I) alone, never on the device.  The forward product and the input gradient g W are
 * regular GEMMs and stay the caller's.  Stateless calls, device pointers, no floating-point atomics, no waits between
 * workgroups; no call synchronises, allocates or reads on the host; every element of every requested output is written.  Two
 * launches.  x and g may have any 4-byte alignment: 16-byte loads are taken where O % 4 == 0, I % 4 == 0 and both bases are
 * 16-byte aligned, scalar loads with the same bits otherwise.
 *
 * Limits (WEKWS_HIP_EINVAL, before any launch, outputs untouched): R >= 1;  1 <= O, I <= 65535;  a grid within 2^31 - 1;  at least
 * one of grad_w and grad_bias;  x and g;  a workspace that is not NULL, 16-byte aligned and at least
 * wekws_hip_linear_wgrad_workspace_bytes(R, O, I) large.
 * ------------------------------------------------------------------------------------------*/
/* Without a device: out = {rows a chain, chains, slices, workgroups of the partial launch, workspace bytes}. */
int wekws_hip_linear_wgrad_plan(int64_t R, int O, int I, int64_t out[5]);
/* Without a device: slices x padded O x padded I doubles and slices x padded O for the bias, rounded up to 16 bytes (padded: to a
 * multiple of 64).  0 on bad arguments. */
size_t wekws_hip_linear_wgrad_workspace_bytes(int64_t R, int O, int I);
int wekws_hip_linear_wgrad(const float* x, const float* g, int64_t R, int O, int I, float* grad_w /* NULL: not wanted */,
                           float* grad_bias /* NULL: not wanted */, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The pointwise (kernel_size 1) Conv1d of the TCN and MDTC blocks, forward and backward: x (B, Ci, T), y and grad_y (B, Co, T),
 * float32, contiguous; w (Co, Ci), the (Co, Ci, 1) weight of nn.Conv1d; bias (Co) or none.  The arithmetic:
 *     forward   y[b][o][t]: acc = +0; i ascending, acc = fmaf(w[o][i], x[b][i][t], acc); then one float32 addition of bias[o]
 *               (none without a bias) -- the exact-float32 matrix instruction from a zeroed accumulator
 *     grad_x    grad_x[b][i][t]: the same chain over o ascending, fmaf(w[o][i], grad_y[b][o][t], acc)
 *     grad_w, grad_bias   wekws_hip_linear_wgrad's contract, unchanged, with rows r = b T + t, R = B T, O = Co, I = Ci: the bits
 *               are those of wekws_hip_linear_wgrad on the (R, Ci) and (R, Co) transposes of x and grad_y, which are not made
 * A (b, t) column's y and grad_x depend on that column alone.  Stateless calls, device pointers, no floating-point atomics, no
 * waits between workgroups; no call synchronises, allocates or reads on the host; every element of every requested output is
 * written.  One launch for the forward; one for grad_x and two for grad_w / grad_bias.  Operands may have any 4-byte alignment:
 * 16-byte loads are taken where T % 4 == 0 (Ci % 4 == 0 for w) and the base is 16-byte aligned, scalar loads with the same bits
 * otherwise.
 *
 * Limits (WEKWS_HIP_EINVAL, before any launch, outputs untouched): B, T >= 1;  1 <= Ci, Co <= 65535;  every grid within 2^31 - 1;
 * no NULL operand;  at least one of the three gradients;  where grad_w or grad_bias is wanted, a workspace that is not NULL,
 * 16-byte aligned and at least wekws_hip_pointwise_conv1d_workspace_bytes(B, Ci, T, Co) large (grad_x alone needs none).
 * ------------------------------------------------------------------------------------------*/
/* Without a device: out = {rows a chain, chains, slices, workgroups of the weight gradient's partial launch, workspace bytes,
 * workgroups of the forward, workgroups of grad_x}; the first five are wekws_hip_linear_wgrad_plan(B T, Co, Ci)'s. */
int wekws_hip_pointwise_conv1d_plan(int B, int Ci, int T, int Co, int64_t out[7]);
/* Without a device: wekws_hip_linear_wgrad_workspace_bytes(B T, Co, Ci).  0 on bad arguments. */
size_t wekws_hip_pointwise_conv1d_workspace_bytes(int B, int Ci, int T, int Co);
int wekws_hip_pointwise_conv1d_forward(const float* x, int B, int Ci, int T, const float* w, const float* bias /* NULL: none */, int Co,
                                       float* y, void* stream);
int wekws_hip_pointwise_conv1d_backward(const float* x, const float* grad_y, int B, int Ci, int T, const float* w, int Co,
                                        float* grad_x /* NULL: not wanted */, float* grad_w /* NULL: not wanted */,
                                        float* grad_bias /* NULL: not wanted */, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The dense (groups 1) dilated Conv1d of the TCN's CnnBlock, forward and backward:
 * F.conv1d(F.pad(x, (left_pad, 0)), w, bias, dilation=dilation) for x (B, Ci, Tin), y and grad_y (B, Co, Tout) with
 * Tout = Tin + left_pad - (K - 1) dilation, float32, contiguous; w (Co, Ci, K) as nn.Conv1d holds it; bias (Co) or none.  The
 * padding's zeros are supplied by the kernels (xp[n < 0] = 0); the padded copy is never made.  The arithmetic:
 *     forward   y[b][o][t]: acc = +0; k ascending and, inside it, i ascending, acc = fmaf(w[o][i][k], xp[b][i][t + k d - left_pad], acc);
 *               then one float32 addition of bias[o] (none without a bias) -- the exact-float32 matrix instruction from a zeroed
 *               accumulator with the reduction index k Ci + i.  The padding's zeros are real operands: an infinite weight over
 *               them is NaN, as in the padded convolution.
 *     grad_x    grad_x[b][i][n]: the same chain over k ascending and, inside it, o ascending,
 *               fmaf(w[o][i][k], grad_y[b][o][n + left_pad - k d], acc), grad_y a zero outside [0, Tout); non-finite weights are
 *               outside the contract here
 *     grad_w, grad_bias   grad_w[:, :, k] is wekws_hip_linear_wgrad's contract, unchanged, with rows r = b Tout + t, R = B Tout,
 *               O = Co, I = Ci and x's row r = xp[b][:, t + k d - left_pad]: the bits of wekws_hip_linear_wgrad on the shifted,
 *               zero-padded, transposed copies, which are not made.  grad_bias is that contract's, computed once.
 * A (b, t) column of y and a (b, n) column of grad_x depend on batch row b alone.  Stateless calls, device pointers, no
 * floating-point atomics, no waits between workgroups; no call synchronises, allocates or reads on the host; every element of
 * every requested output is written.  One launch for the forward; one for grad_x and two for grad_w / grad_bias, whatever K: the
 * taps are a grid dimension.  Operands may have any 4-byte alignment.
 *
 * Limits (WEKWS_HIP_EINVAL, before any launch, outputs untouched): B, Tin >= 1;  1 <= Ci, Co <= 65535;  1 <= K <= 32;
 * dilation >= 1;  (K - 1) dilation + 1 <= 256;  0 <= left_pad <= (K - 1) dilation;  Tout >= 1;  every grid within 2^31 - 1;  no NULL
 * operand;  at least one of the three gradients;  where grad_w or grad_bias is wanted, a workspace that is not NULL, 16-byte
 * aligned and at least wekws_hip_dense_conv1d_workspace_bytes(...) large (grad_x alone needs none).
 * ------------------------------------------------------------------------------------------*/
/* Without a device: out = {rows a chain, chains, slices, workgroups a tap of the weight gradient's partial launch, workspace
 * bytes, workgroups of the forward, workgroups of grad_x, taps (the second grid dimension of the partial and the fold launch),
 * workgroups a tap of the fold launch, Tout}; the first four are wekws_hip_linear_wgrad_plan(B Tout, Co, Ci)'s. */
int wekws_hip_dense_conv1d_plan(int B, int Ci, int Tin, int Co, int K, int dilation, int left_pad, int64_t out[10]);
/* Without a device: K x wekws_hip_linear_wgrad_workspace_bytes(B Tout, Co, Ci).  0 on bad arguments. */
size_t wekws_hip_dense_conv1d_workspace_bytes(int B, int Ci, int Tin, int Co, int K, int dilation, int left_pad);
int wekws_hip_dense_conv1d_forward(const float* x, int B, int Ci, int Tin, const float* w, const float* bias /* NULL: none */, int Co, int K,
                                   int dilation, int left_pad, float* y, void* stream);
int wekws_hip_dense_conv1d_backward(const float* x, const float* grad_y, int B, int Ci, int Tin, const float* w, int Co, int K, int dilation,
                                    int left_pad, float* grad_x /* NULL: not wanted */, float* grad_w /* NULL: not wanted */,
                                    float* grad_bias /* NULL: not wanted */, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WEKWS_HIP_H_ */
