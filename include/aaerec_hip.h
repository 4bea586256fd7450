/*
 * aaerec_hip.h - C ABI of libaaerec_hip.so: the MI355X (gfx950) implementation of the
 * adversarial-autoencoder training step of lgalke/aae-recommender.
 *
 * The reference has no FFI boundary of its own: the hot path sits behind duck-typed Python
 * protocols.  Each entry point below names the reference interface it
 * replaces (file:line, relative to the reference checkout).  INTEGRATION.md shows the ctypes
 * stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every function returns 0 on success or a negative AAE_E* code; aae_last_error() gives
 *     text.  Nothing throws, nothing calls exit().
 *   - all `*_dev` pointers are device pointers on the current HIP device; work is enqueued on
 *     the `stream` argument (a hipStream_t passed as void*; NULL = default stream).  No entry
 *     point synchronises the device except aae_read_losses / aae_load_* / aae_store_*.
 *   - one handle per model replica and per rank; a handle is not thread-safe.
 *   - the caller owns the arena (one device allocation of aae_arena_bytes() bytes, 256-byte
 *     aligned); the library lays out parameters, optimiser state and activations inside it
 *     (aae_tensor_info gives every view), so a host framework can alias them (e.g. as
 *     torch tensors for RCCL collectives) without copies.
 */
#ifndef AAEREC_HIP_H
#define AAEREC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 4 (r6): aae_set_option, aae_ipc_create / _init / _destroy, AAE_ACT_SOFTPLUS .. AAE_ACT_HARDSWISH; no structure changed since 3 */
#define AAE_ABI_VERSION 4

/* error codes */
#define AAE_OK 0
#define AAE_EINVAL (-1)   /* bad argument / unsupported configuration */
#define AAE_ENOMEM (-2)   /* arena too small */
#define AAE_EHIP (-3)     /* a HIP runtime call failed */
#define AAE_ESTATE (-4)   /* call sequence violated (e.g. decode before encode) */

/* activation ids: getattr(nn, activation) in aaerec/aae.py:110 */
enum { AAE_ACT_RELU = 0, AAE_ACT_SELU = 1, AAE_ACT_TANH = 2, AAE_ACT_SIGMOID = 3,
       AAE_ACT_ELU = 4, AAE_ACT_LEAKYRELU = 5,
       /* r6: the other parameter-free element-wise torch.nn classes, at their default arguments.  The layer programs of a model
          with one of them run on the 16-row chain kernel (no 4-row / wide-batch kernel, no fused ranking launch -
          aae_predict_topk takes its two-kernel form): supported, not tuned */
       AAE_ACT_SOFTPLUS = 6, AAE_ACT_HARDTANH = 7, AAE_ACT_RELU6 = 8, AAE_ACT_CELU = 9, AAE_ACT_SOFTSIGN = 10,
       AAE_ACT_HARDSIGMOID = 11, AAE_ACT_LOGSIGMOID = 12, AAE_ACT_SOFTSHRINK = 13, AAE_ACT_HARDSHRINK = 14,
       AAE_ACT_IDENTITY = 15,
       /* ... not monotone: the derivative is evaluated through a branch bit kept in the stored output's last place */
       AAE_ACT_GELU = 16, AAE_ACT_SILU = 17, AAE_ACT_MISH = 18, AAE_ACT_HARDSWISH = 19, AAE_ACT_COUNT = 20 };
/* encoder output activation: PRIOR_ACTIVATIONS, aaerec/aae.py:97-101 */
enum { AAE_FINAL_LINEAR = 0, AAE_FINAL_SOFTMAX = 1, AAE_FINAL_SIGMOID = 2 };
/* TORCH_OPTIMIZERS, aaerec/aae.py:216-219 */
enum { AAE_OPT_ADAM = 0, AAE_OPT_SGD = 1 };
/* where dropout masks and z_real come from */
enum { AAE_RNG_INJECT = 0,   /* caller supplies them (parity tests, reference-RNG mode) */
       AAE_RNG_DEVICE = 1 }; /* counter-based generator inside the kernels */
/* prior for AAE_RNG_DEVICE: PRIOR_SAMPLERS, aaerec/aae.py:90-94 */
enum { AAE_PRIOR_GAUSS = 0, AAE_PRIOR_CATEGORICAL = 1, AAE_PRIOR_BERNOULLI = 2 };
/* which model of the reference the handle trains (cfg.model_kind) */
enum { AAE_MODEL_AAE = 0,    /* AdversarialAutoEncoder, aae.py:587-870 */
       AAE_MODEL_AE = 1,     /* plain AutoEncoder (aae.py:221-458): the step ends after the encoder backward,
                                aae_disc_step / aae_gen_step are errors */
       AAE_MODEL_VAE = 3 };  /* VAE (vae.py:47-266): see aae_vae_step */
/* arithmetic of the GEMM-shaped products (cfg.dtype) */
enum { AAE_DTYPE_F32 = 0,    /* fp32 throughout (the reference's precision) */
       AAE_DTYPE_BF16 = 1 }; /* bf16 matrix-core inputs, fp32 accumulation, fp32 master weights and Adam (config C2) */
/* what happens to gradients */
enum { AAE_GRAD_FUSED = 0,   /* optimiser update fused into the weight-gradient kernels */
       AAE_GRAD_EXPORT = 1 };/* gradients are materialised (data-parallel: all-reduce, then
                                aae_apply_updates) */

/* AdversarialAutoEncoder.__init__ keyword arguments, aaerec/aae.py:588-606, plus sizes that
 * the reference infers in fit() (aae.py:773-793) and build-only knobs. */
typedef struct aae_config {
    int32_t abi_version;      /* AAE_ABI_VERSION */
    int32_t n_items;          /* X.shape[1] */
    int32_t n_hidden;
    int32_t n_code;
    int32_t cond_inc;         /* conditions.size_increment(), 0 without conditions */
    int32_t max_batch;        /* largest number of rows per step / per predict call */
    int32_t max_nnz;          /* largest number of CSR entries in one batch */
    int32_t activation;       /* AAE_ACT_* */
    int32_t enc_final;        /* AAE_FINAL_* */
    int32_t optimizer;        /* AAE_OPT_* */
    int32_t normalize_inputs; /* F.normalize(inp, 1) at aae.py:132-133 */
    int32_t rng_mode;         /* AAE_RNG_* */
    int32_t prior;            /* AAE_PRIOR_* (device rng only) */
    int32_t grad_mode;        /* AAE_GRAD_* */
    float dropout1, dropout2; /* dropout=(.2,.2) */
    float gen_lr, reg_lr;
    float prior_scale;        /* used when has_prior_scale != 0 (aae.py:717-718) */
    int32_t has_prior_scale;
    uint64_t seed;            /* device rng */
    /* build-time knobs of the model (named fields since ABI version 2; they travelled in reserved[0..6] before) */
    int32_t unfused_decoder;  /* 1: keep the decoder output layer on the three-kernel path (A/B measurements, tests) */
    int32_t dp_world;         /* AAE_GRAD_EXPORT: number of data-parallel peers whose packed rows aae_w1_import may
                               * receive (0 = 1) */
    int32_t model_kind;       /* AAE_MODEL_*: which of the reference's models the handle trains */
    int32_t dtype;            /* AAE_DTYPE_*: arithmetic of the matrix-core products (master weights / Adam stay fp32) */
    int32_t blocked_output;   /* 1: batches beyond 112 rows run the fused output layer over row blocks */
    int32_t dense_noise;      /* 1: room for aae_set_input_noise (DenoisingAutoEncoder corrupt='gauss'; needs
                               * model_kind = AAE_MODEL_AE, fp32, fused optimiser) */
    int32_t vae_wide;         /* 1 (model_kind = AAE_MODEL_VAE alone): the VAE's wide bounds - n_hidden <= 1024, n_code <= 512 -
                               * with the per-layer route beyond a chain slot (see aae_vae_step); 0: n_hidden <= 207, 2 * n_code <= 208 */
    int32_t reserved[1];      /* must be zero */
} aae_config;

typedef struct aae_model* aae_handle;

/* A batch = `n_rows` rows picked out of a CSR matrix that is already resident in HBM
 * (replaces X_shuf[start:end].toarray() + torch.FloatTensor(X).cuda(), aae.py:823,751-754).
 * rows_dev == NULL means rows row_start .. row_start+n_rows-1.  Column indices must be unique
 * within a row (canonical CSR, as scipy's tocsr() / sum_duplicates() produce: a repeated (row, item) pair counts
 * once in the BCE target and in the first layer's weight gradient) and values in [0,1] (the reference's BCE raises
 * otherwise). */
typedef struct aae_batch {
    const int64_t* indptr_dev;
    const int32_t* indices_dev;
    const float* values_dev;
    const int32_t* rows_dev;
    int32_t row_start;
    int32_t n_rows;
    int32_t nnz_bound;        /* upper bound on the entries of these rows (<= cfg.max_nnz) */
    int32_t max_row_nnz;      /* upper bound on the entries of any one of these rows; 0 = unknown */
    int64_t generation;       /* ABI 3: caller-supplied id of the CONTENT these pointers name (the CSR arrays and rows_dev): a new
                               * value whenever any of them is rewritten in place or freed and allocated again.  0 = none given.
                               * Only aae_prefetch_batch's matching reads it: a step takes the work built ahead for a named
                               * batch only when pointers, row window AND a non-zero generation are equal. */
} aae_batch;

/* Injected randomness for one partial_fit, in the reference's draw order:
 * keep masks (uint8 0/1, dense row-major [rows][width]) for
 *   0 enc.drop1 1 enc.drop2 2 dec.drop1 3 dec.drop2            (ae_step,  aae.py:687-691)
 *   4 disc.drop1 5 disc.drop2 on z_real, 6,7 the same on z_fake (disc_step, aae.py:724)
 *   8 enc.drop1 9 enc.drop2 10 disc.drop1 11 disc.drop2         (gen_step, aae.py:736-737)
 * and z_real [rows][n_code] BEFORE prior_scale.  A NULL mask = keep everything. */
typedef struct aae_rng_inject {
    const uint8_t* masks_dev[12];
    const float* z_real_dev;
} aae_rng_inject;

/* tensor ids for aae_tensor_info.  Linear layers are stored "augmented": row o holds
 * weight[o, 0:in] followed by bias[o] at column `in`, rows padded to `ld` floats (zeros).
 * The two vocabulary-sized layers are item-major: ENC_W1T row i = enc.lin1.weight[:, i]
 * (bias separate, ENC_B1); DEC_V3 row i = dec.lin3.weight[i, :] ++ dec.lin3.bias[i]. */
enum {
    AAE_T_ENC_W1T = 0, AAE_T_ENC_B1, AAE_T_ENC_W2, AAE_T_ENC_W3,
    AAE_T_DEC_V1, AAE_T_DEC_V2, AAE_T_DEC_V3,
    AAE_T_DISC_D1, AAE_T_DISC_D2, AAE_T_DISC_D3,
    AAE_T_N_PARAMS,
    /* optimiser state: base + 2*param_id (+1 for exp_avg_sq) */
    AAE_T_ADAM_ENC = 16,   /* enc_optim  (aae.py:800), params 0..3 */
    AAE_T_ADAM_GEN = 32,   /* gen_optim  (aae.py:803), params 0..3 */
    AAE_T_ADAM_DEC = 48,   /* dec_optim  (aae.py:801), params 4..6 -> slots 0..2 */
    AAE_T_ADAM_DISC = 64,  /* disc_optim (aae.py:804), params 7..9 -> slots 0..2 */
    /* gradients (AAE_GRAD_EXPORT only), same shapes as the parameters */
    AAE_T_GRAD = 80,       /* + param_id */
    /* activations useful to callers */
    AAE_T_ACT_Z = 96,      /* encoder output of the last encode call [rows][n_code] */
    AAE_T_ACT_LOSSES = 97, /* float[4]: R, D, G of the last step, spare */
    AAE_T_ACT_A1 = 98,     /* first-layer pre-activations of the last encode [rows][n_hidden] */
    AAE_T_ACT_DH2 = 100,   /* the decoder's last hidden activation [rows][n_hidden + 1] (last column = 1: the bias input) */
    AAE_T_ACT_DA2 = 101,   /* dL/d(ACT_DH2) written by aae_output_layer_step, same layout */
    AAE_T_ACT_GA1 = 102,   /* dL/d(ACT_A1) of the last encoder backward [rows][n_hidden] */
    AAE_T_W1_TSYNC = 103,  /* deferred first-layer Adam: int32 [1][n_items] (behind the float view), the last step whose two updates a row
                            * of ENC_W1T has received; read it behind aae_join (a catch-up of the batch named ahead may be writing it) */
    AAE_T_ACT_DZC = 99     /* dL/d(decoder input) of the last ae phase [rows][n_code + cond_inc]: columns n_code.. are
                            * the gradient of the condition block handed to aae_step (trainable conditions) */
};

typedef struct aae_tensor {
    size_t byte_offset;   /* from the arena base */
    int64_t rows, cols;   /* logical shape (cols includes the bias column where augmented) */
    int64_t ld;           /* row stride in floats */
} aae_tensor;

int aae_abi_version(void);
const char* aae_last_error(void);
/* A switch of the library for the handles created FROM NOW ON (value NULL: back to the environment variable AAE_<name>, which
   is what a handle reads otherwise).  Names: struct aae_options, csrc/abi_model.h - paths the parity suites force (NO_CHAIN,
   SPLIT_ANY, BLOCKED_ANY, X16_ROWS, DW_KSPLIT_ROWS, RANK_COLLECT_CAP ...) and the diagnostics of debug runs (DEC_TS ...).  No counterpart in
   the reference (it has no switches: one eager path); a handle reads its switches once, in aae_create. */
int aae_set_option(const char* name, const char* value);

/* construction: the nets + 4 optimisers of fit(), aae.py:782-804 */
int aae_arena_bytes(const aae_config* cfg, size_t* bytes_out);
int aae_create(const aae_config* cfg, void* arena_dev, size_t arena_bytes, void* stream,
               aae_handle* out);
int aae_destroy(aae_handle h);
int aae_tensor_info(aae_handle h, int tensor_id, aae_tensor* out);
/* The Adam updates of ENC_W1T rows whose items are absent from a batch are deferred (they do not
 * depend on the batch) and replayed when a row is next read.  aae_sync replays everything that
 * is pending, after which the arena views of ENC_W1T / ADAM_ENC / ADAM_GEN hold the values an
 * eager implementation would.  aae_load_* / aae_store_* call it themselves. */
int aae_sync(aae_handle h, void* stream);
/* Device RNG (AAE_RNG_DEVICE) under data parallelism: dropout masks and the prior sample are drawn from a counter
 * generator keyed by (seed, step, stream, ROW, column).  With the ranks' handles created with the SAME seed and each
 * told which rows of the global batch it holds - rows [row_offset, row_offset + n_rows) of global_rows - the ranks
 * together draw exactly what one process draws for the whole batch, so 1-GPU and N-GPU runs of a seed are comparable
 * (SURVEY 8e).  (0, 0) = a batch of its own (the default). */
int aae_set_rng_rows(aae_handle h, int64_t row_offset, int64_t global_rows);
/* Call after writing PARAMETER tensors through the arena views of aae_tensor_info (instead of aae_load_linear): the
 * library keeps derived copies of the hidden layers' weights (transposed, for the backward layer chains) and
 * re-derives them before their next use. */
int aae_params_changed(aae_handle h);
/* gen_lr / reg_lr as the exact Python doubles (aae_config carries them as float32) */
int aae_set_lr(aae_handle h, double gen_lr, double reg_lr);

/* nn.Linear state in the reference's state_dict layout (weight [out,in] row-major, bias
 * [out]), host pointers.  Synchronous. net: 0 enc 1 dec 2 disc; layer: 1..3.
 * Either pointer may be NULL: that half is neither read nor written.  A bad net / layer / optimiser id or a NULL handle is
 * AAE_EINVAL and changes nothing.  All four calls may be made at any point between two steps, on a handle that has run: they
 * wait for the handle's side stream (deferred dec_optim launch, a batch's catch-up built ahead), replay the deferred
 * first-layer updates (aae_sync) and invalidate what the library derives from the tensors they write.  A VAE handle's
 * enc.lin3 is [fc21; fc22]: 2 * n_code rows.  Every handle kind carries all nine layers and all four optimisers' tensors
 * (the plain autoencoder's discriminator, the VAE's lin2 layers: stored and loaded, never used). */
int aae_load_linear(aae_handle h, int net, int layer, const float* weight_host,
                    const float* bias_host);
int aae_store_linear(aae_handle h, int net, int layer, float* weight_host, float* bias_host);
/* optimiser state_dict (exp_avg / exp_avg_sq in [out,in] + [out] layout, step count).
 * which: 0 enc_optim 1 dec_optim 2 gen_optim 3 disc_optim.  Any of the four moment pointers may be NULL (left alone);
 * load: step < 0 leaves the count alone, step > 2^31 - 1 is AAE_EINVAL; store: step may be NULL.
 * The step count: every optimiser advances once per training step.  enc_optim and gen_optim update the same tensors and
 * SHARE ONE COUNT - the deferred first-layer updates replay both from one table indexed by it, and it keys the device random
 * generator -, so a count loaded for either is the count of both, of the handle's step counter and of every item's "updated
 * through" step: after loading 5 for enc_optim and then 7 for gen_optim both hold 7.  dec_optim and disc_optim keep counts of
 * their own.  The next step is step count + 1 in every respect (bias corrections, dropout draws, catch-up).
 * cfg.optimizer = AAE_OPT_SGD: the handle carries the same moment tensors and never reads or writes them: store returns what
 * was last loaded (zeros on a new handle), load is a plain round trip, the counts count steps as under Adam. */
int aae_load_adam(aae_handle h, int which, int layer, const float* m_w, const float* v_w,
                  const float* m_b, const float* v_b, int64_t step);
int aae_store_adam(aae_handle h, int which, int layer, float* m_w, float* v_w, float* m_b,
                   float* v_b, int64_t* step);

/* AdversarialAutoEncoder.partial_fit, aae.py:745-766, without conditions or with a constant
 * concatenated condition block cond_dev [rows][cond_inc] (PretrainedWordEmbeddingCondition,
 * condition.py:345-369).  inject may be NULL when cfg.rng_mode == AAE_RNG_DEVICE. */
int aae_step(aae_handle h, const aae_batch* batch, const float* cond_dev,
             const aae_rng_inject* inject, void* stream);

/* The same step cut at the condition boundary, for arbitrary ConditionList plugins whose
 * encode_impose runs in the host framework (condition.py:90-99):
 *   aae_ae_encode          Encoder forward in train mode            (aae.py:687)
 *   [host: zc = conditions.encode_impose(z, cond)]                   (aae.py:688-690)
 *   aae_ae_decode_backward Decoder forward, BCE, decoder backward + dec_optim.step;
 *                          writes dL/dzc [rows][n_code+cond_inc]     (aae.py:692-707)
 *   [host: backprop dzc through the conditions -> dz; conditions.step()]
 *   aae_ae_encoder_backward encoder backward + enc_optim.step        (aae.py:703-706)
 *   aae_disc_gen           disc_step + gen_step                      (aae.py:713-743)
 * The aae_rng_inject handed to a phase stays in force for the later phases of the same step;
 * its device buffers must stay valid until the step's kernels have run. */
int aae_ae_encode(aae_handle h, const aae_batch* batch, const aae_rng_inject* inject,
                  float* z_out_dev, void* stream);
int aae_ae_decode_backward(aae_handle h, const float* zc_dev, int64_t zc_ld,
                           const aae_rng_inject* inject, float* dzc_out_dev, void* stream);
int aae_ae_encoder_backward(aae_handle h, const float* dz_dev, int64_t dz_ld, void* stream);
int aae_disc_gen(aae_handle h, const aae_rng_inject* inject, void* stream);
/* DecodingRecommender.partial_fit, aae.py:489-517 ("only the decoder part of the AAE, basically
 * 2-MLP"): the decoder maps an input block computed by the host's condition plugins to the items.
 *   zin_dev [batch->n_rows][n_code + cond_inc]  the encoded / imposed conditions (aae.py:494-502)
 *   batch                                        the targets y as CSR rows (aae.py:506-507)
 * Decoder forward in train mode, BCE against the batch, decoder backward + its optimiser step
 * (learning rate = cfg.gen_lr); dzin_out_dev (may be NULL) receives dL/dzin for trainable
 * conditions.  Uses masks_dev[2], masks_dev[3] of `inject`.  Predict = aae_decode. */
int aae_decoder_step(aae_handle h, const aae_batch* batch, const float* zin_dev, int64_t zin_ld,
                     const aae_rng_inject* inject, float* dzin_out_dev, void* stream);
/* VAE.partial_fit / VAE.predict, vae.py:147-186, 229-266.  The model must have been created with
 * cfg.model_kind = AAE_MODEL_VAE: ENC_W1T/B1 = fc1, ENC_W3 = [fc21; fc22] (2 * n_code rows: mu, then logvar), DEC_V1 = fc3,
 * DEC_V3 = fc4; ENC_W2 / DEC_V2 / the discriminator are unused; cfg.gen_lr is the single learning rate and
 * cfg.dropout must be (0, 0).  loss = mean BCE (losses[0]) + KL sum (losses[1]), vae.py:132-145.
 * Sizes (aae_arena_bytes / aae_create answer AAE_EINVAL beyond them): n_hidden <= 207, 2 * n_code <= 208 and
 * n_code + cond_inc + 1 <= 1040 - the decoder input [z | condition | 1] runs through fc3 in up to five parts of 208 columns,
 * which holds the reference drivers' conditions (50 + 332 + 1 and, mpd.py, 50 + 932 + 1 columns).
 * cfg.vae_wide = 1 lifts the first two: n_hidden <= 1024, n_code <= 512 (the reference's own grid, vae.py main(): (300, 100)).
 * Such a handle whose sizes fit a chain slot (n_hidden <= 207, 2 * n_code <= 208) is the handle cfg.vae_wide = 0 creates, bit
 * for bit; any other - or any under the NO_CHAIN option - runs its hidden half one launch per layer: every
 * aae_vae_* call works, the ranking and loss calls in their dense form (the *_max_rows calls answer max_batch), and the KL sum is
 * added in a fixed order (the same inputs give the same losses[1] bits).  Every AAE_ACT_* class runs there (none has parameters
 * of its own to train); fp32 only, as every VAE handle.
 *   cond_dev constant concatenated condition block [rows][cond_inc] or NULL
 *   eps_dev   [rows][n_code] standard-normal draws of reparametrize() (vae.py:115-118); NULL = counter generator
 *             (required when cfg.rng_mode == AAE_RNG_INJECT).  The reference samples eps in predict as well. */
int aae_vae_step(aae_handle h, const aae_batch* batch, const float* cond_dev, const float* eps_dev, void* stream);
int aae_vae_predict(aae_handle h, const aae_batch* batch, const float* cond_dev, const float* eps_dev,
                    float* out_dev, int64_t out_ld, void* stream);
/* The VAE step cut at the condition boundary, for ConditionList plugins whose encode_impose runs in the host framework
 * (vae.py:120-130: `z = self.conditions.encode_impose(z, condition_data)` between reparametrize and decode):
 *   aae_vae_encode            x -> fc1 -> (mu, logvar) -> z = mu + eps * exp(logvar / 2) -> z_out_dev [rows][n_code];
 *                             train != 0 opens a training step, 0 = the forward half of VAE.predict (then aae_decode)
 *   [host: zc = conditions.encode_impose(z, c)]
 *   aae_vae_decode_backward   fc3 -> fc4 -> BCE, backward to dzc_out_dev [rows][n_code + cond_inc], fc3 / fc4 updates
 *   [host: backprop dzc through the conditions -> dz; conditions.step()]                              (vae.py:175-181)
 *   aae_vae_encoder_backward  reparametrize' + the KL gradient -> [fc21; fc22] -> fc1, their updates */
int aae_vae_encode(aae_handle h, const aae_batch* batch, const float* eps_dev, float* z_out_dev, int32_t train, void* stream);
int aae_vae_decode_backward(aae_handle h, const float* zc_dev, int64_t zc_ld, float* dzc_out_dev, void* stream);
int aae_vae_encoder_backward(aae_handle h, const float* dz_dev, int64_t dz_ld, void* stream);
/* The ae phase (aae.py:676-711) cut at the decoder's output layer, for vocabulary-sharded data parallelism: the output
 * layer holds ~all of the decoder's parameters and every item receives gradient, so instead of exchanging its
 * [n_items][n_hidden + 1] gradient each rank owns the rows of a slice of the items (a second handle created with
 * n_items = slice size) and the ranks exchange hidden activations, [global rows][n_hidden], instead:
 *   aae_ae_forward         encoder + decoder hidden layers on this rank's documents -> AAE_T_ACT_DH2
 *   [all-gather ACT_DH2 of all ranks into the slice handle's ACT_DH2]
 *   aae_output_layer_step  on the slice handle, batch = the GLOBAL batch restricted to the slice's items (ids rebased):
 *                          logits, BCE (scale: aae_set_grad_scale(slice items / all items)), dV3 + dec_optim on the
 *                          slice's rows, dL/d(dh2) partial -> AAE_T_ACT_DA2; batch = NULL continues the step of
 *                          aae_ae_forward on the same handle (single device: forward + output_layer_step(NULL) +
 *                          backward == the ae phase of aae_step)
 *   [reduce-scatter ACT_DA2 over the ranks -> this rank's rows]
 *   aae_ae_backward        decoder hidden backward + encoder backward + their updates / exported gradients from
 *                          dA2_dev (NULL = this handle's ACT_DA2), leading dimension = ACT_DH2's
 * followed by aae_disc_step / aae_gen_step as in the replicated scheme.  aae_ae_forward / aae_ae_backward: layer-chain models only
 * (n_hidden <= 207, n_code + cond_inc <= 415); the slice handle may be any size. */
int aae_ae_forward(aae_handle h, const aae_batch* batch, const float* cond_dev, const aae_rng_inject* inject, void* stream);
int aae_output_layer_step(aae_handle h, const aae_batch* batch, void* stream);
int aae_ae_backward(aae_handle h, const float* dA2_dev, int64_t dA2_ld, void* stream);
/* ... and the FIRST encoder layer sharded the same way (r2): enc.lin1 is the other [n_items][n_hidden] matrix
 * (reference aae.py:116, 132-135), and under replication its row-sparse gradient is the step's largest exchange (the
 * packed rows of aae_w1_export: ~60 MB gathered per step at 8 x 100 documents).  The slice handle already holds the
 * columns of its items; with these entries it also computes and trains them, and the ranks exchange
 * [global rows][n_hidden] blocks instead (0.6 MB):
 *   aae_set_doc_l1                 slice handle: L1 norms of the COMPLETE documents, indexed by document id (the batch it
 *                                  sees holds only its own columns; F.normalize(x, 1) divides by the whole row,
 *                                  aae.py:133)
 *   aae_set_first_layer_external   replica handle: AAE_T_ACT_A1 is filled by the caller before aae_ae_forward /
 *                                  aae_disc_step, dL/d(a1) of the ae / gen phase is left in AAE_T_ACT_GA1, enc.lin1 is
 *                                  neither read nor updated here; the bias (AAE_T_ENC_B1) stays a small replicated
 *                                  parameter: its gradient is exported with the other small layers'
 *   aae_first_layer_forward        slice handle: its items' share of x * enc.lin1^T for the (global) batch -> its
 *                                  AAE_T_ACT_A1; bias_dev (the replica's AAE_T_ENC_B1) on exactly one share, else
 *                                  NULL.  batch != NULL opens the handle's step
 *                                  (aae_output_layer_step(batch = NULL) continues it), NULL = the running batch again
 *                                  (Enc_eval of disc_step, aae.py:722, after enc_optim's update)
 *   [reduce-scatter the slices' ACT_A1 over the ranks -> the replica's ACT_A1 rows]
 *   [all-gather the replicas' ACT_GA1 -> the slice handle's ACT_GA1]
 *   aae_first_layer_update         slice handle: x^T * dL/d(a1) on its rows of enc.lin1 and optimiser `which` (0
 *                                  enc_optim after the ae phase, 2 gen_optim after gen_step) on them; ga1_dev = NULL:
 *                                  its ACT_GA1, else [rows][ld] - or, rows_per_block > 0, the gathered packets
 *                                  themselves: block r = rows r * rows_per_block .. at ga1_dev + r * block_stride floats
 * aae_prefetch_batch on the slice handle names the NEXT global batch: its distinct-item list and deferred-Adam catch-up
 * then run beside the running step, as for aae_step. */
int aae_set_doc_l1(aae_handle h, const float* doc_l1_dev);
int aae_set_first_layer_external(aae_handle h, int on);
int aae_first_layer_forward(aae_handle h, const aae_batch* batch, const float* bias_dev, void* stream);
int aae_first_layer_update(aae_handle h, const float* ga1_dev, int64_t ld, int32_t rows_per_block, int64_t block_stride,
                           int which, void* stream);
/* The replica's small layers after such an all-gather, in ONE launch: optimiser which_a (0 enc_optim / 2 gen_optim:
 * enc.lin1's bias, enc.lin2, enc.lin3) and, which_b = 1, dec_optim's dec.lin1, dec.lin2 (which_b = -1: none), their
 * gradients read as the sum over the n_peers packets in peer order (bitwise the same on every rank): packet q holds at
 * packets_dev + q * peer_stride + span_offset (floats, multiples of 4) a copy of the arena span that starts at
 * AAE_T_GRAD + AAE_T_ENC_B1.  Replaces a reduction over the peers + aae_apply_updates per optimiser. */
int aae_apply_gathered(aae_handle h, int which_a, int which_b, const float* packets_dev, int64_t peer_stride,
                       int32_t n_peers, int64_t span_offset, void* stream);

/* CategoricalCondition (condition.py:397-508): a trainable embedding of a categorical attribute, reduced over the
 * document's (batch-padded) value list and concatenated to the code.  The table and its optimiser state belong to
 * the caller (plain device arrays [vocab][dim], row-major, dim <= 256); index 0 is the padding / out-of-vocabulary
 * token: it reads as zero and never receives a gradient (nn.Embedding(padding_idx=0)).
 *   idx_dev [rows][width] int32; reduce: sum (also "no reduction" with width = 1) or mean over the padded width
 *   (hid.mean(1), condition.py:485-487, padding included).
 * aae_cat_encode   out_dev[r][0:dim] = reduce_w table[idx[r][w]]   - write it into the cond block of aae_step
 * aae_cat_update   the embedding's backward from dout_dev [rows][>= dim] (AAE_T_ACT_DZC columns of this condition)
 *                  followed by the condition's own optimiser step (condition.py:491-497), default betas / eps:
 *                  AAE_CAT_SPARSE_ADAM  torch.optim.SparseAdam (nn.Embedding(sparse=True), the reference's default):
 *                                       only rows named by the batch move;
 *                  AAE_CAT_ADAM         torch.optim.Adam over the whole table; grad_scratch_dev [vocab][dim] must be
 *                                       zero on the first call and is left zero.
 *                  `step` is the 1-based count of this update (the optimiser's state['step'] after it).
 * Both are aae_bag_encode / aae_bag_update with AAE_BAG_SUM / AAE_BAG_MEAN_WIDTH and padding_idx 0 (the same kernels). */
enum { AAE_CAT_SUM = 0, AAE_CAT_MEAN = 1 };
enum { AAE_CAT_SPARSE_ADAM = 0, AAE_CAT_ADAM = 1 };
int aae_cat_encode(const float* table_dev, int32_t vocab, int32_t dim, const int32_t* idx_dev, int32_t rows,
                   int32_t width, int32_t reduce, float* out_dev, int64_t out_ld, void* stream);
int aae_cat_update(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                   int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width, int32_t reduce,
                   const float* dout_dev, int64_t dout_ld, int32_t optimizer, double lr, int64_t step, void* stream);
/* EmbeddingBagCondition (condition.py:372-394: nn.EmbeddingBag, modes sum / mean / max, over 2-D input) and
 * CategoricalCondition(reduce="max") (hid.max(1)[0]): bags of table rows with a free padding row and the two max
 * reductions (csrc/cond_bag.h).  Handle-free like aae_cat_*: every buffer is the caller's, launches go to `stream`.
 *   padding_idx  -1: no padding row (nn.EmbeddingBag's default; index 0 is an ordinary, trainable row);
 *                >= 0: that row is left out of the reduction and never receives a gradient.
 *                An index outside [0, vocab) is handled like a padding slot.
 *   reduce  AAE_BAG_SUM         sum of the bag
 *           AAE_BAG_MEAN_WIDTH  sum / width, padding counted                             (hid.mean(1))
 *           AAE_BAG_MEAN_COUNT  sum / number of non-padding slots; an empty bag gives 0  (nn.EmbeddingBag(mode="mean"))
 *           AAE_BAG_MAX_PAD0    column-wise maximum in which a padding slot is a candidate of value 0: a row shorter than
 *                               the padded width gives max(..., 0), an all-padding row 0   (hid.max(1)[0])
 *           AAE_BAG_MAX         column-wise maximum of the non-padding slots; an empty bag gives 0
 *                                                                                        (nn.EmbeddingBag(mode="max"))
 *   Tie rule (max modes): the gradient of (row r, column d) goes to the FIRST slot of row r that attains the maximum in
 *   column d; in AAE_BAG_MAX_PAD0 to nobody when that slot is a padding slot.
 *   Recompute contract: aae_bag_update recomputes the winners from the table - the caller must not modify the table
 *   between the aae_bag_encode and the aae_bag_update of a step.  No argmax buffer crosses the step.
 *   optimizer: AAE_CAT_SPARSE_ADAM / AAE_CAT_ADAM as in aae_cat_update.  grad_scratch_dev [vocab][dim] (zero on the
 *   first call, left zero) is needed by AAE_CAT_ADAM and, with either optimiser, by the two max modes.
 *   Limits: dim <= 256, width >= 1, rows * width <= 2^22; the update's duplicate scan is quadratic in rows * width.
 *   Deterministic: no float atomics, the first slot naming a table row sums its contributions in slot order. */
enum { AAE_BAG_SUM = 0, AAE_BAG_MEAN_WIDTH = 1, AAE_BAG_MEAN_COUNT = 2, AAE_BAG_MAX_PAD0 = 3, AAE_BAG_MAX = 4 };
int aae_bag_encode(const float* table_dev, int32_t vocab, int32_t dim, const int32_t* idx_dev, int32_t rows,
                   int32_t width, int32_t reduce, int32_t padding_idx, float* out_dev, int64_t out_ld, void* stream);
int aae_bag_update(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                   int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width, int32_t reduce, int32_t padding_idx,
                   const float* dout_dev, int64_t dout_ld, int32_t optimizer, double lr, int64_t step, void* stream);
/* nn.Embedding's / nn.EmbeddingBag's max_norm and scale_grad_by_freq on the same bags.
 *   aae_bag_renorm  torch's embedding_renorm_, which the module's forward runs first (under no_grad, in training and in eval
 *     alike): every DISTINCT table row named by idx_dev - a padding row too; an index outside [0, vocab) names nothing -
 *     whose p-norm is strictly greater than max_norm is multiplied ONCE by max_norm / (norm + 1e-7), however often it is
 *     named.  Norm, compare, scale and store are fp32; the norm's summation order is fixed (the same bits every run, and
 *     the same bits from aae_bag_csr_renorm).  A launch of its own: call it in front of the aae_bag_encode of the same
 *     idx_dev on the same stream; the encode, the update and the optimiser then see the renormalised table, and the
 *     recompute contract of the max modes holds because nothing touches the table behind the encode.
 *     norm_type: AAE_BAG_NORM_L1, AAE_BAG_NORM_L2 or AAE_BAG_NORM_INF (max |x|).  AAE_EINVAL for max_norm <= 0 and for any
 *     other norm_type.
 *   aae_bag_update_flags  aae_bag_update (which is this call with flags 0) with
 *     AAE_BAG_SCALE_BY_FREQ  the gradient of table row j is divided by the number of times j occurs among ALL indices of the
 *       block (every bag, winners and losers of the max modes alike, whatever the per-sample weights): one IEEE division per
 *       element behind the sum of the row's contributions.  The padding row still gets no gradient.  AAE_CAT_ADAM only
 *       (torch refuses a sparse gradient scaled by frequency): AAE_EINVAL with AAE_CAT_SPARSE_ADAM, and for unknown flags. */
enum { AAE_BAG_NORM_INF = 0, AAE_BAG_NORM_L1 = 1, AAE_BAG_NORM_L2 = 2 };
enum { AAE_BAG_SCALE_BY_FREQ = 1 };
int aae_bag_renorm(float* table_dev, int32_t vocab, int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width,
                   double max_norm, int32_t norm_type, void* stream);
int aae_bag_update_flags(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                         int32_t dim, const int32_t* idx_dev, int32_t rows, int32_t width, int32_t reduce, int32_t padding_idx,
                         const float* dout_dev, int64_t dout_ld, int32_t optimizer, double lr, int64_t step, int32_t flags,
                         void* stream);
/* The same bags from a RESIDENT CSR (csrc/cond_csr.h): the value lists of the whole corpus are uploaded once, a step names
 * its rows, nothing is padded and the update's grouping is a sort - no quadratic scan.
 *   indptr_dev int64 [n_docs + 1], indices_dev int32 [nnz] (table rows), weights_dev float32 [nnz] or NULL
 *   (per_sample_weights: an entry contributes w * table[j], its gradient is w * dout[row]; AAE_BAG_SUM only).  The CSR is NOT
 *   canonical: a row may name a table row several times and the order of its entries is kept.
 *   row_ids_dev int32 [rows] on the device, or NULL for the rows row0 .. row0 + rows.  A row id outside [0, n_docs) is an
 *   empty row.
 *   reduce / padding_idx / optimizer / grad_scratch_dev / lr / step: as in aae_bag_encode / aae_bag_update.  The width of
 *   AAE_BAG_MEAN_WIDTH and AAE_BAG_MAX_PAD0 is the longest list among the step's rows (padding and out-of-range entries
 *   counted, at least 1), computed on the device inside the call's launches.
 *   Same bits as aae_bag_encode / aae_bag_update (and aae_cat_*: AAE_BAG_SUM / AAE_BAG_MEAN_WIDTH with padding_idx 0) on
 *   the same lists padded to that width: the gradient of a table row sums its entries in (row of the batch, position in
 *   the row) order.  The recompute contract of the max modes holds here too.
 *   max_entries: a bound on the entries of the step's rows (<= 2^22; e.g. the sum of the `rows` longest lists of the
 *   corpus).  It sizes the scratch and the number of merge launches; entries beyond it would be dropped.
 *   scratch_dev: 8-byte aligned, at least aae_bag_csr_scratch_bytes(rows, max_entries) bytes (encode: (rows, 0)); its
 *   content is meaningless between calls.  aae_bag_csr_scratch_bytes is arithmetic (no GPU needed); AAE_EINVAL for negative sizes.
 *   Limits: dim <= 256, rows >= 1.  No atomics, no host synchronisation, every launch goes to `stream`. */
int aae_bag_csr_scratch_bytes(int64_t max_rows, int64_t max_entries, int64_t* bytes_out);
int aae_bag_csr_encode(const float* table_dev, int32_t vocab, int32_t dim, const int64_t* indptr_dev,
                       const int32_t* indices_dev, const float* weights_dev, int64_t n_docs, int64_t nnz,
                       const int32_t* row_ids_dev, int64_t row0, int32_t rows, int32_t reduce, int32_t padding_idx,
                       float* out_dev, int64_t out_ld, void* scratch_dev, int64_t scratch_bytes, void* stream);
int aae_bag_csr_update(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                       int32_t dim, const int64_t* indptr_dev, const int32_t* indices_dev, const float* weights_dev,
                       int64_t n_docs, int64_t nnz, const int32_t* row_ids_dev, int64_t row0, int32_t rows,
                       int64_t max_entries, int32_t reduce, int32_t padding_idx, const float* dout_dev, int64_t dout_ld,
                       int32_t optimizer, double lr, int64_t step, void* scratch_dev, int64_t scratch_bytes, void* stream);
/* aae_bag_renorm / aae_bag_update_flags over a window of the resident CSR: the same bits as on the same lists padded.
 *   aae_bag_csr_renorm groups the entries with the update's sort, keyed with no padding row, so a padding-row entry keeps its
 *   table row and that row has an owner too; it takes max_entries (>= 1) and a scratch of
 *   aae_bag_csr_scratch_bytes(rows, max_entries) bytes as aae_bag_csr_update does - no more than that, and no [vocab] marker.
 *   aae_bag_csr_update is aae_bag_csr_update_flags with flags 0. */
int aae_bag_csr_renorm(float* table_dev, int32_t vocab, int32_t dim, const int64_t* indptr_dev, const int32_t* indices_dev,
                       int64_t n_docs, int64_t nnz, const int32_t* row_ids_dev, int64_t row0, int32_t rows, int64_t max_entries,
                       double max_norm, int32_t norm_type, void* scratch_dev, int64_t scratch_bytes, void* stream);
int aae_bag_csr_update_flags(float* table_dev, float* exp_avg_dev, float* exp_avg_sq_dev, float* grad_scratch_dev, int32_t vocab,
                             int32_t dim, const int64_t* indptr_dev, const int32_t* indices_dev, const float* weights_dev,
                             int64_t n_docs, int64_t nnz, const int32_t* row_ids_dev, int64_t row0, int32_t rows,
                             int64_t max_entries, int32_t reduce, int32_t padding_idx, const float* dout_dev, int64_t dout_ld,
                             int32_t optimizer, double lr, int64_t step, int32_t flags, void* scratch_dev,
                             int64_t scratch_bytes, void* stream);
/* PretrainedWordEmbeddingCondition's preprocessing (condition.py:345-369 -> ub.py:52-57, EmbeddedVectorizer.transform:
 * `sparse_scores @ self.embedding`): out_dev[r][0:dim] = sum over the CSR entries e of row r of
 * values[e] * table_dev[indices[e]][0:dim], accumulated in CSR order.  indptr int64 [n_rows + 1] (absolute offsets
 * into indices / values), indices int32, values float32 (the TF-IDF weights); indices outside the table are skipped. */
int aae_csr_embed(const int64_t* indptr_dev, const int32_t* indices_dev, const float* values_dev, int32_t n_rows,
                  const float* table_dev, int32_t n_table_rows, int32_t dim, int64_t table_ld, float* out_dev,
                  int64_t out_ld, void* stream);
/* The constant condition blocks of a batch from matrices RESIDENT in HBM (csrc/cond_gather.h): the document vectors of every
 * PretrainedWordEmbeddingCondition are uploaded once, a step names its rows, and one launch copies them into the step's
 * condition block - nothing of a condition crosses the host inside the loop.  Handle-free like aae_csr_embed and
 * aae_bag_csr_encode: one launch on `stream`, no synchronisation.  For each source s and each row r of the call
 *     out_dev[r * out_ld + col0_s + j] = base_dev_s[id_r * ld_s + j],   0 <= j < width_s
 *   id_r = row_ids_dev[r] (int32 [rows] on the device), or row0 + r when row_ids_dev is NULL: aae_bag_csr_encode's row naming,
 *   so one window of an epoch's permutation serves both.  An id outside [0, n_docs_s) gives a row of zeros (an empty row) and
 *   reads nothing.  Columns of out_dev no source names are not written.  A copy: bit-exact, NaN payloads and -0.0 included.
 *   A source goes by 16-byte loads and stores where both sides allow it - base_dev_s and out_dev on 16 bytes, ld_s, col0_s and
 *   out_ld multiples of 4 -, the columns behind its last full quad one at a time; any other source takes the scalar path.  No
 *   load touches an address outside a source row's [0, width): with ld == width the last row may end with the allocation.
 *   Offsets are 64-bit (id * ld passes 2^31 at a few million documents).
 *   AAE_EINVAL (checked before any HIP call) for n_srcs outside [1, AAE_COND_SRC_MAX], a NULL srcs / out_dev / base_dev,
 *   width < 1, ld < width, n_docs < 0, col0 < 0, col0 + width > out_ld, rows < 0.  rows == 0: nothing is launched.
 *   Sources that overlap in out_dev's columns are the caller's mistake: the order of their stores is not defined. */
#define AAE_COND_SRC_MAX 8
typedef struct { const float* base_dev; int64_t ld; int64_t n_docs; int32_t width; int32_t col0; } aae_cond_src;
int aae_cond_gather(const aae_cond_src* srcs, int32_t n_srcs, const int32_t* row_ids_dev, int64_t row0,
                    int32_t rows, float* out_dev, int64_t out_ld, void* stream);
/* The reference's call form: partial_fit(X) / predict(X) take the DENSE [rows][n_cols] batch that
 * X_shuf[start:end].toarray() produced (aae.py:745-754, 823, 848-853) and upload it whole.  aae_dense_to_csr compacts
 * such a matrix, already on the device as float32 (elem_bytes = 4) or float64 (8), into the CSR form aae_batch takes:
 * indptr_dev int64 [rows + 1], indices_dev int32 / values_dev float32 [capacity], columns ascending within a row.
 * scratch_dev: int32 [rows + 8].  stats_out_host (int32[4], after a stream synchronisation): longest row, total
 * entries, != 0 if a value lies outside [0, 1] (the reference's F.binary_cross_entropy raises on such targets),
 * != 0 if the matrix has more than `capacity` entries (nothing was written). */
int aae_dense_to_csr(const void* dense_dev, int32_t elem_bytes, int64_t ld, int32_t rows, int32_t n_cols,
                     int64_t* indptr_dev, int32_t* indices_dev, float* values_dev, int64_t capacity,
                     int32_t* scratch_dev, int32_t* stats_out_host, void* stream);
/* the two halves of aae_disc_gen (data parallel needs the discriminator update applied
 * between them) */
int aae_disc_step(aae_handle h, const aae_rng_inject* inject, void* stream);
int aae_gen_step(aae_handle h, const aae_rng_inject* inject, void* stream);

/* recon / disc / gen loss of the last step (the three .item() calls, aae.py:711,732,743).
 * Synchronises `stream`. */
int aae_read_losses(aae_handle h, float out_host[3], void* stream);

/* AdversarialAutoEncoder.predict, aae.py:840-870: eval-mode encoder -> (constant concat
 * condition) -> decoder -> sigmoid, out_dev [rows][out_ld] float32. */
int aae_predict(aae_handle h, const aae_batch* batch, const float* cond_dev, float* out_dev,
                int64_t out_ld, void* stream);
/* predict followed on the device by what Evaluation does on the host with the dense matrix:
 * remove_non_missing (row-wise min-max scaling; items present in the input row excluded when
 * exclude_known != 0; evaluation.py:183-199) and argtopk (evaluation.py:20-58).  Writes the k
 * (1 <= k <= min(1024, n_items)) best item ids per row, best first, and their scaled scores: [rows][k].
 * Items of EQUAL fp32 score (saturated sigmoids of a trained model, collisions near 1) are in np.argpartition's arbitrary
 * order in the reference; here the fused form (aae_rank_max_rows) orders them by logit, the dense form by the smaller item
 * id - the k scores are identical, the named items may differ exactly at ties.
 * k > 32 (the reference's MPD driver ranks 500 items per row) takes the long-list kernels (csrc/rank_long.h): the fused form
 * orders by logit, items of equal LOGIT by the smaller id; the dense form by score, then the smaller id.  The output does not
 * vary from run to run.  A row with fewer than k rankable items (exclude_known on a row that names most of the vocabulary)
 * lists its items, then id -1 with score 0 - at every k.  A fused call with k > 32 reads its rows' entry counts back before
 * it returns (it synchronises `stream`; not for stream capture), and ranks a row whose collect list overflowed
 * (RANK_COLLECT_CAP entries, default 4096) through the score matrix in the [max_batch][n_items] scratch: the result is exact
 * either way. */
int aae_predict_topk(aae_handle h, const aae_batch* batch, const float* cond_dev, int32_t k,
                     int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream);
/* Rows ONE aae_predict_topk / aae_decode_topk call may rank (>= max_batch).  Where the fused form applies (r4: the output
 * layer, its sigmoid, the row minimum / maximum, the known-item mask and the top-k selection in one pass over dec.lin3 -
 * the [rows, n_items] score matrix never exists in HBM; hidden widths of the layer-chain kernels) a call takes far more
 * rows than a training batch - the parameter stream is then read once per call, not once per max_batch rows - and such a
 * batch is exempt from the max_batch / max_nnz bounds of aae_batch.  Otherwise *rows_out = max_batch.
 * k > 32 adds a list of 2 x RANK_COLLECT_CAP words per row to the call's workspace and keeps enough workgroups per row block
 * for the floor (32 candidates each, k in all): fewer rows per call than at k <= 32, never fewer than max_batch. */
int aae_rank_max_rows(aae_handle h, int32_t k, int32_t* rows_out);
/* The fused k > 32 calls of this handle since the last read: out[0] calls, [1] rows, [2] rows whose collect list overflowed
 * (ranked through the score matrix instead), [3] entries collected over all rows, [4] the most entries of any row.  Resets
 * the counters.  (How tight the floor is: [3] / [1] against k.) */
int aae_rank_long_stats(aae_handle h, int64_t out[5]);
/* The same behind a decoder input the caller built (AdversarialAutoEncoder.predict's second half, aae.py:855-866:
 * `z = conditions.encode_impose(z, c_batch)` with plugins of any kind, then dec): zc_dev [batch->n_rows][zc_ld],
 * zc_ld >= n_code + cond_inc; `batch` names the input rows (their items are the ones exclude_known removes). */
int aae_decode_topk(aae_handle h, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, int32_t k,
                    int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream);
/* The rank of every held-out item in the FULL ranking of its row - what the unbounded metrics need (mrr, map: RR = 1 / the
 * best rank, AP = mean_j j / r_j over the row's sorted ranks), and everything a metric bounded at k needs as well.  `truth`
 * is a batch over the ground-truth CSR with the row addressing of `batch` (row i of the one belongs to row i of the other;
 * values_dev is not read; max_row_nnz must be given: an upper bound of its longest row).  ranks_out_dev: int32, one entry per
 * stored truth entry of the call's rows, in CSR order (row after row, a row's entries in their stored order): its 1-based
 * rank among the row's items, 0 for an id outside [0, n_items).
 * Tie rule - the ordering of aae_predict_topk: with exclude_known the row's input items are not rankable; the better score
 * first; the fused form (aae_rank_full_max_rows) orders by LOGIT and items of equal logit by the smaller id, exactly the order
 * of aae_predict_topk's lists of k > 20 on the same handle (a truth entry of rank r <= k IS position r - 1 of that list; the
 * lists of k <= 20 may come from another summation order of the same products and differ where two logits are within a
 * rounding of each other); the dense form orders by score, then the smaller id.  A held-out item that is itself a known item
 * ranks behind every rankable item, among the known ones by id: n_rankable + 1 + #{known ids < t}.
 * The fused form answers 8 held-out items per row in two passes over dec.lin3 and repeats them for longer truth rows
 * (csrc/rank_full.h).  Nothing synchronises; the result does not vary from run to run.  As with aae_predict_topk, the hidden
 * layers of a call of more than 224 rows are summed in another order than those of a smaller call: ranks at near-ties may
 * differ between the two (bf16 handles: visibly); calls on one side of 224 rows agree exactly however the rows are chunked. */
int aae_predict_ranks(aae_handle h, const aae_batch* batch, const float* cond_dev, const aae_batch* truth,
                      int32_t exclude_known, int32_t* ranks_out_dev, void* stream);
/* The same behind a decoder input the caller built (as aae_decode_topk): zc_dev [batch->n_rows][zc_ld]. */
int aae_decode_ranks(aae_handle h, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* truth,
                     int32_t exclude_known, int32_t* ranks_out_dev, void* stream);
/* Rows ONE aae_predict_ranks / aae_decode_ranks call may take (>= max_batch; aae_rank_max_rows is about the list calls and
 * keeps its values): the fused form keeps [rows][8] targets and counters instead of candidate lists. */
int aae_rank_full_max_rows(aae_handle h, int32_t* rows_out);
/* The VAE's predict -> rank (reference vae.py:229-266 behind evaluation.py:183-199, 20-58): aae_predict_topk /
 * aae_predict_ranks / aae_decode_topk / aae_decode_ranks / aae_rank_max_rows / aae_rank_full_max_rows for a handle created with
 * cfg.model_kind = AAE_MODEL_VAE (any other handle: AAE_ESTATE; the AAE calls keep what they did on a VAE handle).  Arguments,
 * ordering, tie rules, padding and the rank of a known held-out item are those of the AAE calls; the scores are those of
 * aae_vae_predict for the same rows and the same eps.
 *   eps_dev   [batch->n_rows][n_code] draws of reparametrize(), row i for row i of the batch however the call is carried out
 *             (a k > 32 row that is ranked again through the score matrix reuses its row); NULL = the counter generator
 *             (required when cfg.rng_mode == AAE_RNG_INJECT), whose draw depends on (seed, step, row of the call, column).
 * The fused form (aae_vae_rank_max_rows / aae_vae_rank_full_max_rows rows per call, far more than max_batch) computes the
 * hidden half - fc1, [fc21; fc22], the reparametrisation, the condition block, fc3 - in the call's workspace, 4 rows per
 * workgroup, and ranks over fc4 as the AAE calls do; the [rows, n_items] score matrix never exists.  Its hidden layers are
 * summed in another order than aae_vae_predict's (scores agree to rounding, ids may differ at such near-ties).  A call beyond
 * those rows (<= max_batch then) or on a handle without the rank kernels takes the dense form: aae_vae_predict / aae_decode
 * into the [max_batch][n_items] scratch, ranked there.  The decode calls take a decoder input the caller built
 * (aae_vae_encode(train = 0) -> conditions of any plugin kind), zc_dev [batch->n_rows][zc_ld]. */
int aae_vae_predict_topk(aae_handle h, const aae_batch* batch, const float* cond_dev, const float* eps_dev, int32_t k,
                         int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream);
int aae_vae_predict_ranks(aae_handle h, const aae_batch* batch, const float* cond_dev, const float* eps_dev,
                          const aae_batch* truth, int32_t exclude_known, int32_t* ranks_out_dev, void* stream);
int aae_vae_decode_topk(aae_handle h, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, int32_t k,
                        int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream);
int aae_vae_decode_ranks(aae_handle h, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* truth,
                         int32_t exclude_known, int32_t* ranks_out_dev, void* stream);
int aae_vae_rank_max_rows(aae_handle h, int32_t k, int32_t* rows_out);
int aae_vae_rank_full_max_rows(aae_handle h, int32_t* rows_out);
/* The loss of the model on rows it was not trained on (csrc/loss_eval.h; reference aae.py:176-177, 693-695 - the BCE of
 * F.binary_cross_entropy(x_hat + 1e-12, target + 1e-12) - and vae.py:243-264, loss_function on every test batch), eval mode: no
 * dropout, the weights as they stand, nothing of the handle changes.  Per row of the call
 *   row_bce_dev[i] (double) = the SUM over the n_items cells of row i of the cell loss against `targets`
 * - divide by rows * n_items for the mean the training step reports in aae_read_losses()[0].  `targets` is a batch with the row
 * addressing of `batch` (row i of the one belongs to row i of the other), values in [0, 1], an item at most once per row;
 * NULL = `batch` itself, the reference's choice.  A cell without a target entry is charged softplus(logit) (100 from
 * logit >= 24 ln 2 on, the reference's fp32 saturation), a target entry the reference's form from one logit.
 * Where the fused ranking form applies (aae_loss_max_rows rows per call, far more than max_batch) the [rows, n_items] matrix
 * never exists: one pass over dec.lin3 with the loss epilogue of the rank kernel, the target cells skipped there and charged
 * by a dot product per entry.  Otherwise (<= max_batch rows) the LOGITS go to the [max_batch][n_items] scratch and one
 * workgroup per row sums the same two cell functions.  Sums are fp64 in a fixed order: nothing varies from run to run; two
 * ways of chunking the same rows agree to n_items * 2^-53 relative (calls on one side of 224 rows, as aae_predict_ranks).
 * Nothing synchronises.
 *   aae_decode_loss       the same behind a decoder input the caller built (as aae_decode_topk).
 *   aae_vae_predict_loss  a VAE handle (any other: AAE_ESTATE): eps_dev as in aae_vae_predict_topk; row0 = the counter
 *                         generator's row of the call's first row (the ranking calls count from 0 in every call: pass the
 *                         chunk's first row here and a chunked evaluation draws what one call over all rows draws);
 *                         row_kl_dev[i] (double) = -0.5 sum_c (1 + logvar - mu^2 - exp(logvar)) of row i.
 *   aae_vae_decode_loss   the VAE's decode(zc): no KL term (the caller has the code).
 *   aae_loss_max_rows / aae_vae_loss_max_rows   rows ONE call may take (>= max_batch). */
int aae_predict_loss(aae_handle h, const aae_batch* batch, const float* cond_dev, const aae_batch* targets, double* row_bce_dev,
                     void* stream);
int aae_decode_loss(aae_handle h, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* targets,
                    double* row_bce_dev, void* stream);
int aae_vae_predict_loss(aae_handle h, const aae_batch* batch, const float* cond_dev, const float* eps_dev, int64_t row0,
                         const aae_batch* targets, double* row_bce_dev, double* row_kl_dev, void* stream);
int aae_vae_decode_loss(aae_handle h, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* targets,
                        double* row_bce_dev, void* stream);
int aae_loss_max_rows(aae_handle h, int32_t* rows_out);
int aae_vae_loss_max_rows(aae_handle h, int32_t* rows_out);
/* The item co-occurrence baseline (reference baselines.py:22-43, Countbased: predict = X @ C, C = X^T X of the training set;
 * csrc/cooc.h).  Handle-free like aae_cat_encode / aae_csr_embed: every buffer is the caller's, the launches go to `stream`,
 * nothing synchronises.  `cooc` is C in CSR form with INTEGER values: indptr int64 [n_rows + 1], indices int32 with the columns
 * ascending within a row, values int32.  `batch` names the input rows (values float32 holding whole numbers).
 *   scores[r][j] = sum over the entries (i, x_i) of row r of x_i * C[i][j],   j < n_items
 * summed in int32 and converted to fp32 once: exact (the caller keeps every sum below 2^24; beyond it the fp32 is the rounded
 * integer, beyond 2^31 the sum wraps), identical from run to run and however the rows are chunked.  An input id outside
 * [0, n_items) or >= cooc->n_rows is skipped; an empty input row is a row of zeros.  Columns [n_items, ld) are not written.
 * aae_cooc_scores  the score matrix alone: scores_dev [batch->n_rows][ld], ld >= n_items.
 * aae_cooc_topk    scores into scratch_dev [batch->n_rows][scratch_ld], then the dense form of aae_predict_topk over it
 *                  (csrc/rank_long.h, every k in [1, min(1024, n_items)]): row-wise min-max scaling in which the known items
 *                  still enter the minimum and maximum, known items masked (exclude_known; their ids must then lie in
 *                  [0, n_items), as in every dense ranking call), the better score first and the smaller id at equal scores,
 *                  id -1 / score 0 behind a row's last rankable item.  The scratch is left with the known items at -inf.
 * aae_cooc_ranks   scores into the scratch, then the dense form of aae_predict_ranks (csrc/rank_full.h): one int32 per stored
 *                  entry of the truth rows, CSR order; a truth entry that is a known item ranks behind every rankable item, an
 *                  id outside [0, n_items) ranks 0.  truth->max_row_nnz is not read.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, n_items <= 0, k outside its range,
 * scratch_ld < n_items (or beyond 2^31 - 1), negative row counts, truth->n_rows != batch->n_rows.  No rows: nothing is launched.
 * aae_cooc_scores_i32 / aae_cooc_topk_i32 / aae_cooc_ranks_i32   the same three calls with an int32 score matrix / scratch: the
 *                  int32 sum is stored as it is and ranked AS AN INTEGER, so ids and ranks are exact wherever the sums fit
 *                  int32 - fp32 scores tie from 2^24 on.  Same arguments, same checks, same ordering, padding and truth rules.
 *                  The row minimum and maximum are integers; a scaled score is (float(v) - float(min)) * inv with
 *                  span = float(max) - float(min), inv = span > 0 ? 1 / span : 1, every conversion rounded to nearest.  A known
 *                  item is masked to INT32_MIN (the scratch is left so).  CONTRACT: the caller guarantees that for every row
 *                  sum_i |x_i| * max_j |C[i][j]| < 2^31 (aaerec/cooc.py device_route): then no partial sum wraps and no score
 *                  is INT32_MIN.  The calls do not check it; beyond it sums wrap and a score of INT32_MIN counts as masked. */
typedef struct aae_cooc {
    const int64_t* indptr_dev;
    const int32_t* indices_dev;
    const int32_t* values_dev;
    int32_t n_rows;           /* rows of C (= n_items for X^T X) */
} aae_cooc;
int aae_cooc_scores(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, float* scores_dev, int64_t ld, void* stream);
int aae_cooc_topk(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, int32_t k, int32_t exclude_known,
                  float* scratch_dev, int64_t scratch_ld, int32_t* idx_out_dev, float* val_out_dev, void* stream);
int aae_cooc_ranks(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, const aae_batch* truth, int32_t exclude_known,
                   float* scratch_dev, int64_t scratch_ld, int32_t* ranks_out_dev, void* stream);
int aae_cooc_scores_i32(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, int32_t* scores_dev, int64_t ld, void* stream);
int aae_cooc_topk_i32(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, int32_t k, int32_t exclude_known,
                      int32_t* scratch_dev, int64_t scratch_ld, int32_t* idx_out_dev, float* val_out_dev, void* stream);
int aae_cooc_ranks_i32(const aae_cooc* cooc, int32_t n_items, const aae_batch* batch, const aae_batch* truth, int32_t exclude_known,
                       int32_t* scratch_dev, int64_t scratch_ld, int32_t* ranks_out_dev, void* stream);
/* items per LDS tile of the score kernel (csrc/cooc.h kCoocTile): tests place their shapes across its multiples */
#define AAE_COOC_TILE 16384
/* The exact sparse product behind the co-occurrence matrix (csrc/spgemm.h): C = A . B, A [A->n_rows x p], B [p x n] with
 * p = B->n_rows, every matrix an `aae_cooc` (int64 indptr, int32 indices ascending within a row and without duplicates, int32
 * values); C in the same layout, columns ascending in every row.  Handle-free like the cooc calls; the caller runs the three in
 * this order on one stream and does the scan and the allocation between the last two:
 * aae_spgemm_i32_bound  u_dev [A->n_rows] int64: u_i = sum over the entries (d, .) of A's row i of the stored entries of B's row
 *                       d - the products of row i, an upper bound of its result entries that deals the rows to the two kernels
 *                       (u_i <= AAE_SPGEMM_HASH_PRODUCTS: an LDS hash table; beyond: LDS tiles of AAE_COOC_TILE columns).
 * aae_spgemm_i32_count  row_nnz_dev [A->n_rows] int64: the stored entries of every result row.
 * aae_spgemm_i32_fill   indices_dev / values_dev [indptr[A->n_rows]] from indptr_dev [A->n_rows + 1], the exclusive scan of
 *                       row_nnz_dev; u_dev as Count read it.  Nothing is stored outside a row's own range.
 * Every sum is formed in int32 with integer adds: the same bits every run.  The calls do NOT check for int32 overflow, and the
 * tile kernel takes a cell whose sum is 0 for untouched: the caller guarantees strictly positive values whose sums stay below
 * 2^31 (aaerec/cooc.py device_build_ok).  A column id of A outside [0, p) or of B outside [0, n) is skipped; an empty row of A
 * gives an empty row; A->n_rows = 0 launches nothing.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, a negative size, p > B->n_rows. */
#define AAE_SPGEMM_HASH_PRODUCTS 4096
/* entries of a row of A the tile kernel stages in LDS at a time (csrc/spgemm.h kSpgemmStage): tests give it a longer row */
#define AAE_SPGEMM_STAGE 512
int aae_spgemm_i32_bound(const aae_cooc* A, const aae_cooc* B, int32_t p, int64_t* u_dev, void* stream);
int aae_spgemm_i32_count(const aae_cooc* A, const aae_cooc* B, int32_t n, const int64_t* u_dev, int64_t* row_nnz_dev, void* stream);
int aae_spgemm_i32_fill(const aae_cooc* A, const aae_cooc* B, int32_t n, const int64_t* u_dev, const int64_t* indptr_dev,
                        int32_t* indices_dev, int32_t* values_dev, void* stream);
/* Transpose of a canonical CSR matrix (csrc/sptrans.h): T = A^T for A [n_rows x n_cols] - int64 indptr, int32 indices ascending
 * within a row and without duplicates, 4-byte values that are moved as raw bits (int32 and float32 alike) - T in the same layout,
 * its rows ascending and duplicate-free: the indptr, indices and value bits of scipy's A.T.tocsr() after sort_indices(), the same
 * bits every run.  Handle-free like the spgemm calls; the caller runs the two in this order on one stream and does the scan and
 * the allocation between them:
 * aae_csr_transpose_count  col_nnz_dev [n_cols] int64 (zeroed by the call): the stored entries of every column of A.
 * aae_csr_transpose_fill   t_indices_dev / t_values_dev [nnz] from t_indptr_dev [n_cols + 1], the exclusive scan of col_nnz_dev.
 *                          cursor_dev [n_cols] int64 is scratch (zeroed by the call).  A row of T of more than AAE_SPTRANS_LDS
 *                          entries is sorted through scratch_dev, `scratch_pairs` 8-byte (row, value) pairs: nnz > AAE_SPTRANS_LDS
 *                          requires scratch_pairs >= nnz (nnz = t_indptr[n_cols], passed by the caller who sized the result).
 * A column id outside [0, n_cols) is skipped; nothing is stored outside a row's own range [t_indptr[c], t_indptr[c + 1]); every
 * loop is bounded, so a wrong t_indptr drops entries and does not hang.  n_rows = 0 or n_cols = 0 launches nothing.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, a negative size, a scratch that is too
 * small or not 8-byte aligned. */
#define AAE_SPTRANS_LDS 4096
int aae_csr_transpose_count(const int64_t* indptr_dev, const int32_t* indices_dev, int32_t n_rows, int32_t n_cols,
                            int64_t* col_nnz_dev, void* stream);
int aae_csr_transpose_fill(const int64_t* indptr_dev, const int32_t* indices_dev, const void* values_dev, int32_t n_rows,
                           int32_t n_cols, const int64_t* t_indptr_dev, int32_t* t_indices_dev, void* t_values_dev,
                           int64_t* cursor_dev, void* scratch_dev, int64_t scratch_pairs, int64_t nnz, void* stream);
/* Mutual information of a contingency table that is never stored (reference utils.py:10-71, compute_mutual_info; csrc/mutinfo.h):
 * C = A . B with the operands of the spgemm calls - A = X^T [A->n_rows x p], B = Y [p x n], p = B->n_rows, strictly positive int32
 * values - and scikit-learn's mutual_info_score(contingency=C) in the per-row form
 *   MI = (1/T) sum_i [ S1_i + pi_i (ln T - ln pi_i) ],  S1_i = sum_j c_ij (ln c_ij - ln pj_j),  pi_i = sum_j c_ij,  T = sum_i pi_i
 * with pj_j = sum_d B_dj a_d, a_d = sum_i A_id.  c_ij is int32; a, pi, pj and T are int64; every logarithm and sum is fp64.
 * Handle-free like the spgemm calls; the caller runs aae_spgemm_i32_bound and then the three in this order on one stream:
 * aae_mi_i32_marginals  a_dev [p] and pj_dev [n] int64 (zeroed by the call, then integer atomics: the same bits every run),
 *                       lnpj_dev [n] fp64 = log((double)pj_j), 0 where pj_j = 0 (the row pass never reads such an entry).
 * aae_mi_i32_rows       row_s1_dev [A->n_rows] fp64 = S1_i and row_pi_dev [A->n_rows] int64 = pi_i: row i of C is accumulated in
 *                       LDS exactly as aae_spgemm_i32_fill accumulates it (u_dev deals the rows to the same two paths) and
 *                       reduced there in a fixed order - the same bits every run.  An empty row writes 0 and 0.
 * aae_mi_i32_finish     out_dev, 16 bytes, 8-byte aligned: double mi = max(sum / T, 0) at byte 0, int64 T at byte 8; the row
 *                       terms are summed by one workgroup in a fixed order.  T = 0 (m = 0 included) gives mi = 0, not NaN.
 * CONTRACT (aaerec/utils.py device_mi_ok; not checked by the calls): canonical operands, every c_ij < 2^31, T < 2^53 - then
 * every marginal is an exact double.  A column id of A outside [0, p) or of B outside [0, n) is skipped; A->n_rows = 0 launches
 * no row kernel.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, a negative size, p > B->n_rows, an
 * out_dev that is not 8-byte aligned. */
int aae_mi_i32_marginals(const aae_cooc* A, const aae_cooc* B, int32_t p, int32_t n, int64_t* a_dev, int64_t* pj_dev,
                         double* lnpj_dev, void* stream);
int aae_mi_i32_rows(const aae_cooc* A, const aae_cooc* B, int32_t n, const int64_t* u_dev, const double* lnpj_dev,
                    double* row_s1_dev, int64_t* row_pi_dev, void* stream);
int aae_mi_i32_finish(int32_t m, const double* row_s1_dev, const int64_t* row_pi_dev, void* out_dev, void* stream);
/* The most-popular baseline (reference baselines.py:46-58, MostPopular: predict = the item counts of the training set, the same
 * vector for every row; csrc/popular.h).  Handle-free like the cooc calls: every buffer is the caller's, the launches go to
 * `stream`, nothing synchronises.  Every row ranks the same scores, so the items are ordered ONCE by the caller and a row only
 * leaves its known items out: no [rows][n_items] scratch, no limit on a row's known items, every k in [1, n_items].
 * aae_pop_counts  counts_dev [n_items] int32 (overwritten: zeroed by the call, then integer atomics - the same bits every run):
 *                 counts[j] = sum over the rows d of X of x_dj, X the training matrix in the `aae_cooc` layout (int32 values).
 *                 A column id outside [0, n_items) is skipped.  CONTRACT (not checked): max_j sum_d |x_dj| < 2^31.
 * `aae_popular`   counts_dev as above; order_dev [n_items] int32, the item ids by (count descending, id ascending); pos_dev
 *                 [n_items] int32, its inverse (pos[order[i]] = i).  The caller builds the last two from the first.
 * aae_pop_topk    idx_out_dev / val_out_dev [batch->n_rows][k]: a row's list is the first k items of `order` that are not among
 *                 its known items (exclude_known; otherwise the first k of `order`) - the better score first and the smaller id
 *                 at equal scores, as in every ranking call - id -1 / score 0 behind its last rankable item.  A scaled score is
 *                 the min-max scaling over ALL items, known ones included, with the fp32 formula of aae_cooc_topk_i32:
 *                 (float(v) - float(min)) * inv, span = float(max) - float(min), inv = span > 0 ? 1 / span : 1, where
 *                 min = counts[order[n_items - 1]] and max = counts[order[0]].
 * aae_pop_ranks   one int32 per stored entry of the truth rows, CSR order: 1 + the number of items ordered before it,
 *                 1 + pos[t] - #{known j : pos[j] < pos[t]}.  A truth entry that is a known item ranks behind every rankable
 *                 item, among the known items by id: 1 + (n_items - m) + #{known j < t} for a row of m known items.  A truth id
 *                 outside [0, n_items) ranks 0 and pos_dev is not read for it.  truth->max_row_nnz is not read.
 * CONTRACT for both ranking calls, as in every dense ranking call: the ids of a batch row lie in [0, n_items) and ascend without
 * duplicates.  The values of `batch` and `truth` are not read (values_dev may be NULL); row_start / rows_dev address rows as in
 * every aae_batch.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, n_items <= 0, k outside [1, n_items],
 * negative row counts, truth->n_rows != batch->n_rows.  No rows: nothing is launched. */
typedef struct aae_popular {
    const int32_t* counts_dev;
    const int32_t* order_dev;
    const int32_t* pos_dev;
    int32_t n_items;
} aae_popular;
int aae_pop_counts(const aae_cooc* X, int32_t n_items, int32_t* counts_dev, void* stream);
int aae_pop_topk(const aae_popular* pop, const aae_batch* batch, int32_t k, int32_t exclude_known, int32_t* idx_out_dev,
                 float* val_out_dev, void* stream);
int aae_pop_ranks(const aae_popular* pop, const aae_batch* batch, const aae_batch* truth, int32_t exclude_known,
                  int32_t* ranks_out_dev, void* stream);
/* The random baseline (reference baselines.py:7-19, RandomBaseline: predict = rand(rows, items); csrc/randrank.h) from the
 * library's keyed generator.  Handle-free like the pop calls: every buffer is the caller's, the launches go to `stream`, nothing
 * synchronises, and no [rows][n_items] scratch exists on the ranking calls: a draw is regenerated wherever it is needed.
 *   key    = rng_key(seed, draw, 0) ^ 15 * 0xA0761D6478BD642F      (stream 15 of the generator, csrc/device_common.h)
 *   s(r,j) = hash_cell(key, r, j) >> (32 - bits)                    (an integer in [0, 2^bits))
 *   score  = s * 2^-bits                                            (exact in fp32)
 * for item j of row r = row0 + the row of the call: the row's index in the caller's WHOLE test set, so that a call over rows
 * [a, b) with row0 = a computes what those rows of one call over everything compute.  `batch` addresses the known items of the
 * call's rows as in every aae_batch (row_start / rows_dev; its values are not read, values_dev may be NULL).
 * aae_rand_scores  out_dev [n_rows][ld] fp32, ld >= n_items: the scores.
 * aae_rand_topk    idx_out_dev / val_out_dev [batch->n_rows][k], k in [1, min(1024, n_items)]; val_out_dev may be NULL.  A row's
 *                  list: the k items it does not know (exclude_known; otherwise of all items) with the largest s, the larger s
 *                  first and the smaller id at equal s, as in every ranking call - an exact two-level radix select over the
 *                  bits-bit values, the candidate buffer bounded by k; id -1 / score 0 behind its last rankable item.  A scaled
 *                  score is the min-max scaling over ALL items of the row, known ones included, in fp32:
 *                  (score - min) * inv, span = max - min, inv = span > 0 ? 1 / span : 1.
 * aae_rand_ranks   one int32 per stored entry of the truth rows, CSR order: 1 + #{i not known, i != j, s_i > s_j or (s_i == s_j
 *                  and i < j)}.  A truth entry that is a known item ranks behind every rankable item, among the known items by id:
 *                  1 + (n_items - m) + #{known j < t} for a row of m known items; a truth id outside [0, n_items) ranks 0 - both
 *                  as in aae_pop_ranks.  truth->max_row_nnz bounds the entries of a truth row (0 = unknown: 4096 is assumed); a
 *                  row that holds more entries than the bound it was given ranks 0 throughout.
 * CONTRACT for both ranking calls, as in every dense ranking call: the ids of a batch row lie in [0, n_items) and ascend without
 * duplicates.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, n_items <= 0, k out of range, bits outside
 * [1, 24], a negative draw, row0 or row count, row0 + rows beyond 2^31, ld < n_items, truth->n_rows != batch->n_rows,
 * truth->max_row_nnz > 4096.  No rows: nothing is launched. */
int aae_rand_scores(uint64_t seed, int64_t draw, int64_t row0, int32_t bits, int32_t n_items, int32_t n_rows, float* out_dev,
                    int64_t ld, void* stream);
int aae_rand_topk(uint64_t seed, int64_t draw, int64_t row0, int32_t bits, int32_t n_items, const aae_batch* batch, int32_t k,
                  int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream);
int aae_rand_ranks(uint64_t seed, int64_t draw, int64_t row0, int32_t bits, int32_t n_items, const aae_batch* batch,
                   const aae_batch* truth, int32_t exclude_known, int32_t* ranks_out_dev, void* stream);
/* Ranking metrics from held-out ranks (csrc/rank_metrics.h).  Handle-free like the calls above: every buffer is the caller's, the
 * launches go to `stream`, nothing synchronises.  With a row's stored ranks in ascending order r_1 <= ... <= r_m - entries order by
 * (rank, position in the row) - and h = #{r_j <= k}:
 *   AAE_METRIC_MRR    1 / r_1 if r_1 <= k, else 0                          (replaces reference evaluation.py:94-115 with
 *   AAE_METRIC_MAP    (sum_{j <= h} j / r_j) / h, 0 if h = 0                rank_metrics_with_std.py mean_reciprocal_rank,
 *   AAE_METRIC_P      h / k                                                 average_precision; evaluation.py:118-164)
 *   AAE_METRIC_NDCG   (sum_{j <= h} d[r_j]) / (sum_{i = 1 .. min(k, m)} d[i])   (replaces eval/mpd/mpd_metrics.py:53-119)
 *   AAE_METRIC_RPREC  #{r_j <= min(m, k)} / m                               (replaces eval/mpd/mpd_metrics.py:43-51)
 *   AAE_METRIC_CLICKS floor((r_1 - 1) / 10) if r_1 <= k, else k / 10 + 1    (replaces eval/mpd/mpd_metrics.py:133-144)
 * k = 0 means unbounded and is defined for MRR and MAP only.  A row without entries scores 0, CLICKS k / 10 + 1.  A stored rank
 * AAE_RANK_ABSENT is "not retrieved": it counts towards m and satisfies no r <= k, unbounded kinds included.  A row of more than
 * AAE_METRIC_ROW_MAX entries, or with a rank below 1, is NaN in every metric; its neighbours are not touched.
 * aae_metric_rows    (replaces evaluation.py:94-164, rank_metrics_with_std.py and eval/mpd/mpd_metrics.py:43-144 per row)
 *                    rows: int64 indptr_dev [n_rows + 1] and int32 ranks_dev in CSR order, as the aae_*_ranks calls write them
 *                    (item-id order within a row, not ascending).  specs: a HOST array of n_metrics in [1, AAE_METRIC_MAX].
 *                    discounts_dev [n_discounts] fp64: d[i] at index i - 1, the caller's table (the reference's is
 *                    1 / log2(1 + i)); read by NDCG specs only, may be NULL without one.  per_row_dev [n_metrics][ld] fp64,
 *                    ld >= n_rows.  Sums run one term after the other in ascending j: the same bits every run.
 * aae_metric_finish  (replaces the (mean, std) of evaluation.py:160-163 and rank_metrics_with_std.py: np.mean, np.std)
 *                    out_dev [n_metrics][2] fp64: the mean and the population standard deviation of the n_rows values of each
 *                    metric - two passes (the mean, then the mean of the squared deviations, then sqrt), one workgroup per metric,
 *                    a fixed reduction shape, no float atomics.  n_rows = 0 gives NaN.
 * aae_ranks_from_lists  (replaces the relevance lookup of evaluation.py:80-91 on lists; eval/mpd/mpd_metrics.py:43-144 take lists)
 *                    ids_dev [truth->n_rows][ld] int32, a row's list its first k ids, best first, -1 padding as the *_topk calls
 *                    write it.  truth: the canonical truth rows (ids ascending without duplicates; values not read).
 *                    ranks_out_dev: one int32 per stored truth entry, CSR order of the call's rows: position + 1 of the entry in
 *                    its row's list - the smaller one for an id listed twice - or AAE_RANK_ABSENT.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, a negative size, n_metrics out of range,
 * an unknown kind, k < 0, k = 0 on a kind without an unbounded form, an NDCG spec with k above n_discounts, ld too small, a
 * negative truth->row_start without rows_dev. */
#define AAE_METRIC_MAX 32
#define AAE_METRIC_ROW_MAX 4096
#define AAE_RANK_ABSENT 2147483647
typedef enum aae_metric_kind {
    AAE_METRIC_MRR = 0, AAE_METRIC_MAP = 1, AAE_METRIC_P = 2, AAE_METRIC_NDCG = 3, AAE_METRIC_RPREC = 4, AAE_METRIC_CLICKS = 5
} aae_metric_kind;
typedef struct aae_metric_spec {
    int32_t kind;             /* aae_metric_kind */
    int32_t k;                /* the cap; 0 = unbounded (MRR, MAP) */
} aae_metric_spec;
typedef struct aae_rank_rows {
    const int64_t* indptr_dev;
    const int32_t* ranks_dev;
    int32_t n_rows;
} aae_rank_rows;
int aae_metric_rows(const aae_rank_rows* rows, const aae_metric_spec* specs, int32_t n_metrics, const double* discounts_dev,
                    int32_t n_discounts, double* per_row_dev, int64_t ld, void* stream);
int aae_metric_finish(const double* per_row_dev, int64_t ld, int32_t n_rows, int32_t n_metrics, double* out_dev, void* stream);
int aae_ranks_from_lists(const int32_t* ids_dev, int64_t ld, int32_t k, const aae_batch* truth, int32_t* ranks_out_dev, void* stream);
/* The truncated-SVD baseline (reference svd.py:15-57, SVDRecommender: predict = (X V^T) V[:, :n_items], V = TruncatedSVD's
 * components_ [dims][n_features], n_features = items (+ the tf-idf vocabulary of the titles); csrc/lowrank.h).  Handle-free like
 * the cooc calls.  `lowrank` is ONE fp32 table for both products: vt_dev [n_features][ld], row f = column f of V, ld a multiple
 * of 4 floats >= dims rounded up to 4 (the padding zero), 16-byte aligned, dims in [1, AAE_LOWRANK_DIMS_MAX].
 *   hidden[r][d] = sum over the entries (f, x_f) of row r of `features` of x_f * vt[f][d]     (CSR order, one fmaf per term)
 *   scores[r][j] = sum over d of hidden[r][d] * vt[j][d],   j < n_items <= n_features           (fp32 matrix pipe, d ascending)
 * Both are k-ordered fp32 fmaf chains that depend on the row alone: the same bits from run to run and however the rows are
 * chunked.  |scores - exact| <= 2^-24 (dims + nnz_r + 4) sum_d (sum_f |x_f| |V_df|) |V_dj| to first order (csrc/lowrank.h).
 * A feature id outside [0, n_features) is skipped; an empty row is a row of zeros.  hidden_dev [features->n_rows][hidden_ld]
 * is the caller's scratch for the hidden vectors (hidden_ld >= dims, a multiple of 4 floats, 16-byte aligned; columns
 * [dims, hidden_ld) are not written and not used).  Columns [n_items, ld) of the score matrix are not written.
 * aae_lowrank_scores  the score matrix alone: scores_dev [features->n_rows][ld], ld >= n_items, a multiple of 4 floats, 16-byte
 *                     aligned.
 * aae_lowrank_topk    scores into scratch_dev [rows][scratch_ld] (as ld above), then the dense form of aae_predict_topk over it
 *                     exactly as aae_cooc_topk: `items` names the known items of the same rows (ids in [0, n_items) when
 *                     exclude_known, as in every dense ranking call; its values are not read), row-wise min-max scaling with
 *                     the known items still in the extrema, the better score first and the smaller id at equal scores, id -1 /
 *                     score 0 behind a row's last rankable item, k in [1, min(1024, n_items)].
 * aae_lowrank_ranks   scores into the scratch, then the dense form of aae_predict_ranks as aae_cooc_ranks: one int32 per stored
 *                     entry of the truth rows, CSR order.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, dims / n_features / n_items out of range,
 * k outside its range, a leading dimension that is too small or not a multiple of 4 floats, a misaligned base, negative row
 * counts, items->n_rows or truth->n_rows != features->n_rows.  No rows: nothing is launched. */
typedef struct aae_lowrank {
    const float* vt_dev;      /* [n_features][ld] */
    int64_t ld;
    int32_t n_features;
    int32_t dims;
} aae_lowrank;
int aae_lowrank_scores(const aae_lowrank* lowrank, int32_t n_items, const aae_batch* features, float* hidden_dev, int64_t hidden_ld,
                       float* scores_dev, int64_t ld, void* stream);
int aae_lowrank_topk(const aae_lowrank* lowrank, int32_t n_items, const aae_batch* features, const aae_batch* items, int32_t k,
                     int32_t exclude_known, float* hidden_dev, int64_t hidden_ld, float* scratch_dev, int64_t scratch_ld,
                     int32_t* idx_out_dev, float* val_out_dev, void* stream);
int aae_lowrank_ranks(const aae_lowrank* lowrank, int32_t n_items, const aae_batch* features, const aae_batch* items,
                      const aae_batch* truth, int32_t exclude_known, float* hidden_dev, int64_t hidden_ld, float* scratch_dev,
                      int64_t scratch_ld, int32_t* ranks_out_dev, void* stream);
/* widest hidden vector of the projection kernel (csrc/lowrank.h kProjDimsMax) */
#define AAE_LOWRANK_DIMS_MAX 4096
/* The projection of the calls above as a product of its own: out[r][0:width] = sum over the entries (f, x_f) of row r of `rows`
 * of x_f * dense[f][0:width] - a tall CSR x row-major dense product, the same kernel, the same k-ordered fmaf chain in CSR order
 * and the same bits however it is launched (the randomized range finder of aaerec/lowrank.py is built from it).  dense_dev
 * [n_cols][ld] and out_dev [rows->n_rows][ld_out]: leading dimensions in multiples of 4 floats on 16-byte aligned bases,
 * ld >= width rounded up to 4 (the padding is read, its products are not stored), ld_out >= width; width in
 * [1, AAE_LOWRANK_DIMS_MAX].  An id outside [0, n_cols) is skipped; an empty row is a row of zeros; columns [width, ld_out) are
 * not written.  AAE_EINVAL as above. */
int aae_spmm_f32(const aae_batch* rows, const float* dense_dev, int64_t ld, int32_t n_cols, int32_t width, float* out_dev,
                 int64_t ld_out, void* stream);
/* IRGAN (reference irgan/cf_gan.py, gen_model.py, dis_model.py; csrc/irgan.h).  Handle-free like the calls above: every buffer is
 * the caller's, the launches go to `stream`, nothing synchronises.  A net is three fp32 tensors and their momentum buffers:
 * user_emb [users][dim], item_emb [items][dim], item_bias [items], rows contiguous; dim in [1, AAE_IRGAN_DIM_MAX].
 *   logit(u, j) = item_bias[j] + sum_d user_emb[u][d] * item_emb[j][d]      (one fmaf chain, d ascending, from the bias)
 * Momentum SGD as torch.optim.SGD(lr, momentum): buf = momentum * buf + grad, p -= lr * buf, on EVERY element of all three tensors
 * on every step (the reference's gradients are dense).  fp32 parameters and products, no float atomics, duplicates summed in list
 * order, reductions over the items in one fixed order with fp64 sums: the same inputs give the same bits.
 * scratch_dev / scratch_bytes of the training calls: 256-byte aligned, at least aae_irgan_scratch_bytes(net) (a fixed region and
 * the softmax tables of one user); aae_irgan_sample_neg works on as many users at once as further table slots fit.
 * aae_irgan_scores     out_dev [n_rows][ld] fp32 (ld as in aae_lowrank_scores): logit(users_dev[r], j), and exactly 0 where j is a
 *                      training positive of that user - pos_indptr_dev int64 [users + 1] / pos_items_dev int32, ascending ids per
 *                      user, both NULL for none.  A user id outside [0, users) gives a row of zeros.
 * aae_irgan_topk       scores of the known->n_rows users into scratch_dev [rows][scratch_ld], then the dense form of
 * aae_irgan_ranks      aae_predict_topk / aae_predict_ranks over it exactly as aae_lowrank_topk / _ranks: `known` names the known
 *                      items of the TEST rows (masked when exclude_known), min-max scaling, the smaller id at equal scores, -1 / 0
 *                      tails, k in [1, min(1024, items)].
 * aae_irgan_d_steps    n_steps consecutive D steps over lines_dev int32 [n_lines][3] = (user, positive, negative): step s takes
 *                      lines [s batch_size, min((s + 1) batch_size, n_lines)), each line the triples (u, pos, 1), (u, neg, 0);
 *                      loss = mean BCE-with-logits + lambda (mean(user_emb^2) + mean(item_emb^2) + mean(item_bias^2)), written
 *                      to losses_out_dev [n_steps] fp64 when that is not NULL.  batch_size in [1, AAE_IRGAN_BATCH_MAX].
 * aae_irgan_sample_neg generate_for_d for users users_dev[0 .. n_users): user q owns lines [line_off_dev[q], line_off_dev[q + 1])
 *                      (at most max_pos <= AAE_IRGAN_POS_MAX of them) and gets one negative per line, written to column 2, drawn
 *                      from softmax(logit / temperature) by the keyed generator: stream 16, keyed by (seed, draw, user id, index
 *                      of the line within the user) - the same lines under any chunking of the users (sampler: csrc/irgan.h).
 * aae_irgan_g_steps    one G step per entry of users_dev [n_steps], in order: p = softmax(logit), n = 2 |pos| samples - injected
 *                      (samples_dev int32, step s at sample_off_dev[s], int64 [n_steps + 1]) or, both NULL, drawn from the mixture
 *                      0.8 p + 0.2 uniform(pos) on stream 17 keyed by (seed, draw, user id, sample index) -, reward_s = 2
 *                      (sigmoid(dis logit) - 1/2) p_s / pn_s with pn_s = 0.8 p_s + 0.2 / |pos| [s in pos], loss = -mean(log(max(p_s,
 *                      1e-8)) reward_s) to losses_out_dev [n_steps] fp64 if given; samples_out_dev (with sample_off_dev), if given,
 *                      receives the samples every step used.  pos_*: the ascending positives by user id, at
 *                      most max_pos per user; a user without positives takes no step.
 * AAE_EINVAL (with aae_last_error) before anything touches the device: a NULL pointer, dim outside [1, 64], users or items not
 * positive, k out of range, a bad ld or base, batch_size outside [1, 1024], n_steps beyond the lines, max_pos above 2048, a
 * temperature that is not positive, a scratch that is too small or misaligned. */
#define AAE_IRGAN_DIM_MAX 64
#define AAE_IRGAN_POS_MAX 2048
#define AAE_IRGAN_BATCH_MAX 1024
#define AAE_IRGAN_TILE 128
typedef struct aae_irgan_net {
    float* user_emb_dev;      /* [users][dim] */
    float* item_emb_dev;      /* [items][dim] */
    float* item_bias_dev;     /* [items] */
    float* m_user_emb_dev;    /* the momentum buffers, same shapes (the training calls; the scoring calls do not read them) */
    float* m_item_emb_dev;
    float* m_item_bias_dev;
    int32_t users;
    int32_t items;
    int32_t dim;
} aae_irgan_net;
int aae_irgan_scratch_bytes(const aae_irgan_net* net, size_t* bytes_out);
int aae_irgan_scores(const aae_irgan_net* gen, const int32_t* users_dev, int32_t n_rows, const int64_t* pos_indptr_dev,
                     const int32_t* pos_items_dev, float* out_dev, int64_t ld, void* stream);
int aae_irgan_topk(const aae_irgan_net* gen, const int32_t* users_dev, const int64_t* pos_indptr_dev, const int32_t* pos_items_dev,
                   const aae_batch* known, int32_t k, int32_t exclude_known, float* scratch_dev, int64_t scratch_ld,
                   int32_t* idx_out_dev, float* val_out_dev, void* stream);
int aae_irgan_ranks(const aae_irgan_net* gen, const int32_t* users_dev, const int64_t* pos_indptr_dev, const int32_t* pos_items_dev,
                    const aae_batch* known, const aae_batch* truth, int32_t exclude_known, float* scratch_dev, int64_t scratch_ld,
                    int32_t* ranks_out_dev, void* stream);
int aae_irgan_d_steps(const aae_irgan_net* dis, const int32_t* lines_dev, int64_t n_lines, int32_t batch_size, int32_t n_steps, float lr,
                      float momentum, float lambda, double* losses_out_dev, void* scratch_dev, size_t scratch_bytes, void* stream);
int aae_irgan_sample_neg(const aae_irgan_net* gen, const int32_t* users_dev, const int64_t* line_off_dev, int32_t n_users, int32_t max_pos,
                         float temperature, uint64_t seed, int64_t draw, int32_t* lines_dev, int64_t n_lines, void* scratch_dev,
                         size_t scratch_bytes, void* stream);
int aae_irgan_g_steps(const aae_irgan_net* gen, const aae_irgan_net* dis, const int32_t* users_dev, int32_t n_steps,
                      const int64_t* pos_indptr_dev, const int32_t* pos_items_dev, int32_t max_pos, const int32_t* samples_dev,
                      const int64_t* sample_off_dev, int32_t* samples_out_dev, uint64_t seed, int64_t draw, float lr, float momentum,
                      double* losses_out_dev, void* scratch_dev, size_t scratch_bytes, void* stream);
/* split form for generic conditions */
int aae_encode(aae_handle h, const aae_batch* batch, float* z_out_dev, void* stream);
int aae_decode(aae_handle h, const float* zc_dev, int64_t zc_ld, int32_t n_rows,
               float* out_dev, int64_t out_ld, void* stream);

/* data parallel (AAE_GRAD_EXPORT): after the caller has all-reduced the AAE_T_GRAD tensors of
 * optimiser `which` (0 enc 1 dec 2 gen 3 disc), apply torch.optim.Adam/SGD.step to them. */
int aae_apply_updates(aae_handle h, int which, void* stream);
/* Row-sparse exchange of the first encoder layer's gradient (only the rows of the items in the
 * batch are non-zero).  aae_w1_export packs this rank's rows into hdr_dev (int32[1 + cap]: count,
 * then item ids) and vals_dev (float[cap][n_hidden]) and clears them; after an all-gather the
 * caller hands the n_peers packets (peer p at byte offset p * peer_stride_bytes from both base
 * pointers) to aae_w1_import, which sums them in peer order, brings the union of rows up to date
 * and runs the optimiser `which` (0 enc_optim after the ae phases, 2 gen_optim after gen_step) on
 * them.  cfg.dp_world must hold the number of peers. */
int aae_w1_export(aae_handle h, int32_t* hdr_dev, float* vals_dev, int32_t cap, void* stream);
/* packet layout for `cap` rows: hdr_words int32 words of header, then cap * n_hidden floats of
 * rows, then the encoder's small-layer gradients (b1, W2, W3), which aae_w1_import also sums and
 * applies - so one all-gather per exchange point carries everything the encoder optimisers need */
int aae_w1_packet_floats(aae_handle h, int32_t cap, int64_t* hdr_words, int64_t* total_floats);
int aae_w1_import(aae_handle h, const int32_t* hdr_dev, const float* vals_dev, int32_t cap, int32_t n_peers,
                  int64_t peer_stride_bytes, int which, void* stream);
/* Sharded optimiser: aae_apply_updates_except is aae_apply_updates without tensor
 * `skip_tensor_id`; aae_apply_shard runs optimiser `which` on rows [row_begin, row_end) of that
 * tensor with the caller's gradient shard (e.g. a reduce-scatter result).  Used for DEC_V3:
 * reduce-scatter -> update 1/world of the rows -> all-gather the updated rows. */
int aae_apply_updates_except(aae_handle h, int which, int skip_tensor_id, void* stream);
int aae_apply_shard(aae_handle h, int tensor_id, int64_t row_begin, int64_t row_end,
                    const float* grad_shard_dev, int which, void* stream);
/* ---- the data-parallel step as ONE call (r3; SURVEY 8b "aae_comm_init + entry points that enqueue kernels and RCCL calls") ----
 * Scheme: both vocabulary-wide matrices sharded over the ranks (aae_first_layer_* / aae_output_layer_step above; DESIGN.md
 * 5.0): per partial_fit the ranks exchange seven small blocks - reduce-scatter of the first layer's shares, all-gather of
 * the decoder's last hidden activations, reduce-scatter of dL/d(hidden), all-gather of [dL/d(a1) | small-layer gradients]
 * (twice: enc_optim, gen_optim), reduce-scatter for Enc_eval, all-reduce of the discriminator's gradients.  aae_dp_step
 * enqueues ALL of it - kernels and collectives - on `stream`; no host work in between (driven phase by phase from Python
 * the loop needed 0.35 ms of host time per step at 8 ranks against 0.33 ms of GPU work).
 * The collectives come as a table of function pointers over device float buffers: count = floats PER RANK (all_gather:
 * what each rank sends; reduce_scatter: what each rank receives, sums over the ranks; all_reduce: the whole buffer, in
 * place); each enqueues on `stream` and returns 0 or a negative AAE_E* code.  aae_rccl_init fills the table with RCCL
 * (xGMI) collectives on a communicator the library creates from a 128-byte ncclUniqueId (rank 0: aae_rccl_unique_id, then
 * hand it to the other ranks by any means - torch.distributed.broadcast, MPI, a file); librccl.so is opened at run time.
 * Any other table works as well (the tests use host-staged gloo collectives and single-process stand-ins).
 *   replica            this rank's replica handle: grad_mode = AAE_GRAD_EXPORT, aae_set_first_layer_external(1)
 *   slice              this rank's item-slice handle (fused optimiser, aae_set_doc_l1, aae_set_grad_scale(slice / all items))
 *   local              this rank's documents (its share of the global batch) in the replica's corpus
 *   global_slice       the GLOBAL batch, rank-major, in the slice's corpus (its items' columns); n_rows = world x local's
 *   next_global_slice  the global batch of the NEXT step (aae_prefetch_batch on the slice handle) or NULL
 *   cond_dev / inject  as aae_step */
typedef struct aae_collectives {
    void* ctx;
    int (*all_gather)(void* ctx, const float* send_dev, float* recv_dev, int64_t count, void* stream);
    int (*reduce_scatter)(void* ctx, const float* send_dev, float* recv_dev, int64_t count, void* stream);
    int (*all_reduce)(void* ctx, float* buf_dev, int64_t count, void* stream);
    int32_t world, rank;
} aae_collectives;
int aae_rccl_unique_id(char id_out[128]);
int aae_rccl_init(const char id[128], int32_t world, int32_t rank, aae_collectives* out);
int aae_rccl_destroy(aae_collectives* c);
/* set-up: the replica's scratch for the gathered packets of `world` ranks x n_rows local documents (else aae_dp_step
 * allocates it in its first call) */
int aae_dp_reserve(aae_handle replica, int32_t n_rows, int32_t world);
int aae_dp_step(aae_handle replica, aae_handle slice, const aae_collectives* coll, const aae_batch* local,
                const aae_batch* global_slice, const aae_batch* next_global_slice, const float* cond_dev,
                const aae_rng_inject* inject, void* stream);
/* The third data-parallel scheme (r4): ONE handle per rank = its item slice of the two vocabulary-wide layers
 * + a full copy of the hidden layers, the WHOLE global batch through the hidden stacks on every rank (identical inputs ->
 * identical small-layer gradients and updates: no gradient exchange), and three all-reduces of [global rows, n_hidden]
 * partial sums per partial_fit (the first layer's pre-activations, dL/d(dh2), the first layer again for Enc_eval) - against 7
 * collectives, gradient packets and a second handle in aae_dp_step.  north_star's "RCCL all-reduce ... over xGMI": these are
 * the only all-reduces the step needs.  Reference: aae.py:745-766 over the global batch.
 *   handle      fused optimiser, aae_set_first_layer_external(1), aae_set_doc_l1, max_batch = the global batch
 *   batch       the GLOBAL batch in the handle's corpus (its items' columns); next_batch: named ahead (aae_prefetch_batch) or NULL
 *   item_share  items of this handle / items of the model (the BCE is a mean over all items)
 *   cond_dev    the condition block of ALL rows; inject as aae_step (masks / z_real of all rows) */
int aae_shard_step(aae_handle h, const aae_collectives* coll, const aae_batch* batch, const aae_batch* next_batch,
                   const float* cond_dev, const aae_rng_inject* inject, float item_share, void* stream);
/* r6: the same table as a ONE-SHOT all-reduce over peer-mapped mailboxes, for the ranks of one node and the small exchanges of
 * aae_shard_step (csrc/ipc_collectives.h): every rank copies its operand into its own mailbox, publishes the call, waits for
 * its peers' flags and adds the world mailboxes in rank order - one launch, one hop over xGMI, the same bits on every rank.
 * all_reduce only (all_gather / reduce_scatter fail: aae_dp_step's exchanges are RCCL's).  No counterpart in the reference.
 *   aae_ipc_create   allocates this rank's mailbox for operands of up to max_floats floats; handle_out: 64 bytes
 *                    (hipIpcMemHandle_t) for the caller to carry to every peer (torch.distributed all_gather)
 *   aae_ipc_init     handles = world x 64 bytes in rank order (this rank's own entry is not read); maps the peers' mailboxes
 *   aae_ipc_destroy  after a barrier of the caller's (no peer may still read this rank's mailbox); reports a wait that timed out */
int aae_ipc_create(int64_t max_floats, char handle_out[64], void** mailbox_out);
int aae_ipc_init(void* mailbox, const char* handles, int32_t world, int32_t rank, int64_t max_floats, aae_collectives* out);
int aae_ipc_destroy(aae_collectives* c, void* mailbox);
/* a single-process stand-in table (measurement aid: one rank's compute with every exchange replaced by device copies of the
 * same shapes - all_gather = the operand repeated `world` times, reduce_scatter = its first chunk, all_reduce = identity;
 * rank 0 of `world`) */
int aae_echo_collectives(int32_t world, aae_collectives* out);
/* blocking copy between any two buffers (host or device) behind `stream`: what a host-side collectives table needs to
 * stage operands without a HIP binding of its own */
int aae_memcpy_sync(void* dst, const void* src, size_t bytes, void* stream);

/* scale applied to this rank's loss gradients (local_rows / global_rows) so that the
 * all-reduced sum equals the single-process mean over the global batch. */
int aae_set_grad_scale(aae_handle h, float scale);

/* Live per-kernel timing for bench.py's roofline line: when enabled, a hipEvent pair is
 * recorded on the launch stream around each launch of the kernels below; aae_profile_read
 * waits for them, returns the summed duration and resets the counter. */
enum { AAE_K_ENC_GATHER = 0,   /* sparse row gather of the first encoder layer */
       AAE_K_DEC_BCE_FWD,      /* decoder output GEMM + sigmoid/BCE epilogue */
       AAE_K_DEC_DA2,          /* dL/dlogits * V3 (split-K) */
       AAE_K_DEC_DV3_ADAM,     /* dV3 GEMM + fused Adam on V3 */
       AAE_K_ENC_W1_ADAM,      /* Adam over the touched rows of the encoder's first layer */
       AAE_K_DEC_FUSED,        /* fused decoder output layer: logits + BCE + dV3/Adam + dA2 (B <= ~104) */
       AAE_K_CHAIN,            /* a layer-chain program: the hidden stacks of one phase (5 launches per step) */
       AAE_K_DEC_CRIT,         /* split form of the fused output layer, critical launch: logits + BCE + dA2 (+ dL/dlogits tiles) */
       AAE_K_DEC_OPT,          /* ... deferred launch on the library's side stream: dV3 + dec_optim behind the rest of the step */
       AAE_K_RANK,             /* fused predict -> rank: output layer + sigmoid + min/max + known-item mask + per-workgroup top-k;
                                * k > 32: also floor + collect + sort, and the dense form's long-list kernel */
       AAE_K_COLLECTIVE,       /* a collective of aae_dp_step / aae_shard_step: event pair on the step's stream around the table's call
                                * (what the rank waits: the transfer AND the slowest rank's arrival) */
       AAE_K_UNIQ_ITEMS,       /* uniq_items_kernel as a launch of its own: a batch's distinct-item list (a list built by workgroups of
                                * a layer-chain launch is no launch and is not counted) */
       AAE_K_W1_CATCHUP,       /* w1_catchup_kernel as a launch of its own: the deferred first-layer Adam replayed on listed (or all) rows */
       AAE_K_VAE_REPARAM,      /* vae_reparam_fwd_kernel / vae_reparam_bwd_kernel: the reparametrisation of a VAE handle on the per-layer
                                * route (cfg.vae_wide; a layer-chain program carries it as an op and is counted as AAE_K_CHAIN) */
       AAE_K_N };
/* on = 0: off; 1: every kernel id above; otherwise a selection: bit (k + 1) of `on` times kernel id k
 * (an event pair costs a few microseconds of stream time, so a timed run selects only what it reports) */
int aae_profile_enable(aae_handle h, int on);
int aae_profile_read(aae_handle h, int kernel_id, double* total_ms, int64_t* launches);

/* The fused decoder output layer (B <= ~104, fused optimiser) runs as TWO launches: what the rest of the step waits
 * for (logits, BCE, dL/d(hidden)) on the caller's stream, and the weight gradient + dec_optim pass over DEC_V3 - work
 * only the NEXT step's forward needs (reference aae.py:709 `self.dec_optim.step()` followed by aae.py:713-743, which
 * never read dec) - on a stream the handle owns, concurrently with the rest of the step.  Every entry point of this
 * library that touches DEC_V3, its moments or the step's scratch first makes its `stream` wait for that launch, so
 * callers that go through the ABI see the reference's ordering.  A caller that reads DEC_V3 / ADAM_DEC + 4,5 through
 * its own arena views (aae_tensor_info) calls aae_join first: it makes `stream` wait for the deferred launch (a
 * no-op when none is pending).  aae_sync includes it.  aae_set_split(h, 0) turns the split form off (one launch,
 * everything on the caller's stream: needed to capture a step into a hipGraph without joining), n > 0 sets the number
 * of workgroups of the deferred launch (default: by shape - enough for the launch to take ~80 us, at most 9/16 of the
 * CUs in fp32, 5/8 with bf16 inputs). */
/* DenoisingAutoEncoder(corrupt='gauss'), reference dae.py:40-45 and 191: `self.enc(self.corrupt(batch, noise_factor))`
 * with gauss_noise = batch + randn(batch.size()) * noise_factor - the encoder of the NEXT step-opening call reads the
 * DENSE batch plus noise_dev [rows][noise_ld >= n_items] (already scaled) on all n_items columns, L1-normalised over all
 * of them (aae.py:132-133); its first layer runs as a dense product, its weight gradient as a dense product with the
 * optimiser on every row of ENC_W1T.  The BCE target stays the clean batch.  Needs cfg.dense_noise = 1 (room for the
 * dense input; plain autoencoder, fp32, fused optimiser); noise_dev must stay valid until the step has run. */
int aae_set_input_noise(aae_handle h, const float* noise_dev, int64_t noise_ld);
/* The same corruption drawn from the device generator (cfg.rng_mode == AAE_RNG_DEVICE, else AAE_ESTATE), so that cfg.seed
 * determines it and no [rows][n_items] noise block exists in memory: the NEXT step-opening call's encoder reads the dense
 * batch plus scale x N(0, 1), cell (r, j) = scale * gauss(word stream 14 of the opened step, r, j) with the product in
 * fp32, r the row of the GLOBAL batch as dropout places it (aae_set_rng_rows), j the item.  Same contract as
 * aae_set_input_noise: needs cfg.dense_noise = 1, holds for one step, cleared when the step opens.  A pointer set by
 * aae_set_input_noise and a pending request of this call replace each other: the later call wins. */
int aae_set_input_noise_gen(aae_handle h, float scale);
/* DenoisingAutoEncoder(corrupt='zeros'), reference dae.py:48-52 (`batch[rand(batch.size()) < noise_factor] = 0`), on the
 * entries of a CSR matrix [n_rows, *] in device memory, from the device generator (cfg.rng_mode == AAE_RNG_DEVICE, else
 * AAE_ESTATE):  out_values[e] = keep ? values[e] : 0  for every entry e of rows [0, n_rows), entry (r, j) kept iff
 * word(cfg.seed, step, stream 13, r, j) >= min(2^32 - 1, p * 2^32) - the dropout rule, p in [0, 1] the DROP probability
 * (p == 0 keeps everything).  r is the row's index in the matrix handed over, j the item id, step is *step counter* + 1
 * read on the device in stream order: the value of the first training step that can read the thinned matrix.  int64
 * indptr (indptr[0] need not be 0: entries are addressed by indptr's values), int32 indices, float32 values;
 * out_values_dev == values_dev is allowed.  One launch of a fixed grid whatever n_rows is. */
int aae_dae_thin(aae_handle h, const int64_t* indptr_dev, const int32_t* indices_dev, const float* values_dev, int64_t n_rows,
                 float p, float* out_values_dev, void* stream);
int aae_join(aae_handle h, void* stream);
/* ... the deferred optimiser launch alone: enough before reading or writing the AAE_T_ACT_* tensors (a prefetch started
 * with aae_prefetch_batch touches enc.lin1 and its bookkeeping only and keeps running). */
int aae_join_output_layer(aae_handle h, void* stream);
/* The epoch loop (aae.py:808-831) knows the batch AFTER the one it is about to run.  Named here before the step that
 * precedes it (aae_step / aae_ae_encode / aae_ae_forward), that batch's share of the step-opening work - the list of
 * its distinct items and the replay of the deferred zero-gradient Adam steps on their enc.lin1 rows (what
 * torch.optim.Adam did eagerly in enc_optim.step() / gen_optim.step(), aae.py:706,742) - runs on the handle's side
 * stream while the step before it executes, instead of opening the next step.  A hint, not a promise: a next step on
 * any other batch (other pointers / row window) ignores it and does the work itself.
 * The step recognises the named batch by its pointers, its row window and aae_batch.generation (ABI 3; r1-r4 went by the
 * pointers alone, and a buffer refilled in place or re-allocated at the same address was silently taken for the batch
 * whose item list had been built ahead - rows missing from that list got no update).  The caller bumps `generation`
 * whenever it rewrites or re-allocates any array the batch names; a batch with generation 0 is never matched, and naming
 * one here is accepted and ignored.  What stays the caller's duty is what any asynchronous reader asks: the named arrays
 * must stay allocated and unchanged until the work built from them has run (the step after the next, or aae_join).
 * grad_mode = fused only (otherwise accepted and ignored). */
int aae_prefetch_batch(aae_handle h, const aae_batch* next);
int aae_set_split(aae_handle h, int32_t workgroups);

#ifdef __cplusplus
}
#endif
#endif /* AAEREC_HIP_H */
