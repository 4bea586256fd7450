"""ctypes binding of libaaerec_hip.so (C ABI: include/aaerec_hip.h).

PyTorch is used for plumbing only: it owns the HBM arena (one uint8 tensor), gives the
current HIP stream and lets parameter / gradient views be handed to torch.distributed
(RCCL).  All arithmetic of the AAE step runs in the hand-written gfx950 kernels.

There is NO CPU fallback: importing this module without the built library, or creating a
model without a GPU, raises.
"""
import ctypes as C
import itertools
import weakref
import os

import numpy as np
import torch  # must be imported before the library so both share one HIP runtime

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AAE_HIP_LIB") or os.path.join(_HERE, "libaaerec_hip.so")     # (AAE_HIP_LIB: A/B builds of the library)

ABI_VERSION = 4
# getattr(nn, activation)() of the reference (aae.py:110): the parameter-free element-wise classes of torch.nn at their default
# arguments (r6: 6-19).  Classes with parameters, state or a row-wise definition (PReLU, RReLU, Threshold, GLU, Softmax,
# Softmin, LogSoftmax, MultiheadAttention ...) and Tanhshrink have no kernel: HipAAE raises with this list.
ACTIVATIONS = {"ReLU": 0, "SELU": 1, "Tanh": 2, "Sigmoid": 3, "ELU": 4, "LeakyReLU": 5,
               "Softplus": 6, "Hardtanh": 7, "ReLU6": 8, "CELU": 9, "Softsign": 10, "Hardsigmoid": 11, "LogSigmoid": 12,
               "Softshrink": 13, "Hardshrink": 14, "Identity": 15, "GELU": 16, "SiLU": 17, "Mish": 18, "Hardswish": 19}
FINALS = {"linear": 0, "softmax": 1, "sigmoid": 2}
OPTIMIZERS = {"adam": 0, "sgd": 1}
PRIORS = {"gauss": 0, "categorical": 1, "bernoulli": 2}
RNG_INJECT, RNG_DEVICE = 0, 1
VAE_CHAIN_HIDDEN_MAX, VAE_CHAIN_CODE2_MAX = 207, 208      # a VAE handle without cfg.vae_wide: n_hidden, 2 * n_code (one chain slot)
VAE_WIDE_HIDDEN_MAX, VAE_WIDE_CODE_MAX = 1024, 512        # ... with it (csrc/abi_model.h kVaeWideHiddenMax / kVaeWideCodeMax)
RANK_K_MAX = 1024         # longest list of predict_topk / decode_topk (aaerec_hip.h; beyond 32: csrc/rank_long.h)
COOC_TILE = 16384         # items per LDS tile of the co-occurrence score kernel (AAE_COOC_TILE; csrc/cooc.h kCoocTile)
SPGEMM_HASH_PRODUCTS = 4096   # most products of a row the sparse product keeps in an LDS hash table (AAE_SPGEMM_HASH_PRODUCTS; csrc/spgemm.h)
SPGEMM_STAGE = 512        # entries of a row of A its tile kernel stages in LDS at a time (AAE_SPGEMM_STAGE)
SPTRANS_LDS = 4096        # longest row of a transpose sorted in LDS in one go (AAE_SPTRANS_LDS; csrc/sptrans.h): longer ones merge through a scratch
IRGAN_DIM_MAX, IRGAN_POS_MAX, IRGAN_BATCH_MAX, IRGAN_TILE = 64, 2048, 1024, 128      # AAE_IRGAN_* (csrc/irgan.h)
LOWRANK_DIMS_MAX = 4096   # widest hidden vector of the truncated-SVD projection kernel (AAE_LOWRANK_DIMS_MAX; csrc/lowrank.h)
METRIC_MAX = 32           # most metric specs of one aae_metric_rows call (AAE_METRIC_MAX; csrc/rank_metrics.h)
METRIC_ROW_MAX = 4096     # longest row of held-out ranks the metric kernel sorts in LDS (AAE_METRIC_ROW_MAX)
RANK_ABSENT = 2 ** 31 - 1  # the stored rank of a held-out item a list does not hold (AAE_RANK_ABSENT)
METRIC_NDCG_K_MAX = 1 << 20    # longest discount table the wrapper builds and uploads: an ndcg@k beyond it is the host's
METRIC_KINDS = {"mrr": 0, "map": 1, "p": 2, "ndcg": 3, "r-prec": 4, "clicks": 5}        # aae_metric_kind
GRAD_FUSED, GRAD_EXPORT = 0, 1


class _NullCtx:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NULL_CTX = _NullCtx()

# tensor ids (aaerec_hip.h)
T_ENC_W1T, T_ENC_B1, T_ENC_W2, T_ENC_W3, T_DEC_V1, T_DEC_V2, T_DEC_V3, T_DISC_D1, T_DISC_D2, T_DISC_D3 = range(10)
T_ADAM_ENC, T_ADAM_GEN, T_ADAM_DEC, T_ADAM_DISC, T_GRAD = 16, 32, 48, 64, 80
T_ACT_Z, T_ACT_LOSSES, T_ACT_A1, T_ACT_DZC, T_ACT_DH2, T_ACT_DA2 = 96, 97, 98, 99, 100, 101
T_ACT_GA1 = 102
T_W1_TSYNC = 103
CAT_SUM, CAT_MEAN = 0, 1
CAT_SPARSE_ADAM, CAT_ADAM = 0, 1
BAG_SUM, BAG_MEAN_WIDTH, BAG_MEAN_COUNT, BAG_MAX_PAD0, BAG_MAX = range(5)
BAG_NORM_TYPES = {float("inf"): 0, 1.0: 1, 2.0: 2}      # norm_type -> AAE_BAG_NORM_INF / _L1 / _L2: the norms the renorm kernels have
BAG_SCALE_BY_FREQ = 1                                    # AAE_BAG_SCALE_BY_FREQ
O_ENC, O_DEC, O_GEN, O_DISC = 0, 1, 2, 3
MODEL_AAE, MODEL_AE, MODEL_VAE = 0, 1, 3          # cfg.model_kind
DTYPE_F32, DTYPE_BF16 = 0, 1                      # cfg.dtype


class AaeConfig(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("n_items", C.c_int32), ("n_hidden", C.c_int32),
                ("n_code", C.c_int32), ("cond_inc", C.c_int32), ("max_batch", C.c_int32),
                ("max_nnz", C.c_int32), ("activation", C.c_int32), ("enc_final", C.c_int32),
                ("optimizer", C.c_int32), ("normalize_inputs", C.c_int32), ("rng_mode", C.c_int32),
                ("prior", C.c_int32), ("grad_mode", C.c_int32), ("dropout1", C.c_float),
                ("dropout2", C.c_float), ("gen_lr", C.c_float), ("reg_lr", C.c_float),
                ("prior_scale", C.c_float), ("has_prior_scale", C.c_int32), ("seed", C.c_uint64),
                ("unfused_decoder", C.c_int32), ("dp_world", C.c_int32), ("model_kind", C.c_int32),
                ("dtype", C.c_int32), ("blocked_output", C.c_int32), ("dense_noise", C.c_int32),
                ("vae_wide", C.c_int32), ("reserved", C.c_int32 * 1)]


class AaeBatch(C.Structure):
    _fields_ = [("indptr_dev", C.c_void_p), ("indices_dev", C.c_void_p), ("values_dev", C.c_void_p),
                ("rows_dev", C.c_void_p), ("row_start", C.c_int32), ("n_rows", C.c_int32),
                ("nnz_bound", C.c_int32), ("max_row_nnz", C.c_int32), ("generation", C.c_int64)]


class AaeRngInject(C.Structure):
    _fields_ = [("masks_dev", C.c_void_p * 12), ("z_real_dev", C.c_void_p)]


_COLL_AG = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)
_COLL_AR = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p)


class AaeCollectives(C.Structure):
    """aae_collectives (include/aaerec_hip.h): the collectives aae_dp_step calls at its exchange points."""
    _fields_ = [("ctx", C.c_void_p), ("all_gather", _COLL_AG), ("reduce_scatter", _COLL_AG), ("all_reduce", _COLL_AR),
                ("world", C.c_int32), ("rank", C.c_int32)]


class AaeTensor(C.Structure):
    _fields_ = [("byte_offset", C.c_size_t), ("rows", C.c_int64), ("cols", C.c_int64), ("ld", C.c_int64)]


class AaeCooc(C.Structure):
    _fields_ = [("indptr_dev", C.c_void_p), ("indices_dev", C.c_void_p), ("values_dev", C.c_void_p), ("n_rows", C.c_int32)]


class AaeCondSrc(C.Structure):
    """aae_cond_src: one resident constant condition block of an aae_cond_gather call."""
    _fields_ = [("base_dev", C.c_void_p), ("ld", C.c_int64), ("n_docs", C.c_int64), ("width", C.c_int32), ("col0", C.c_int32)]


class AaePopular(C.Structure):
    _fields_ = [("counts_dev", C.c_void_p), ("order_dev", C.c_void_p), ("pos_dev", C.c_void_p), ("n_items", C.c_int32)]


class AaeMetricSpec(C.Structure):
    _fields_ = [("kind", C.c_int32), ("k", C.c_int32)]


class AaeRankRows(C.Structure):
    _fields_ = [("indptr_dev", C.c_void_p), ("ranks_dev", C.c_void_p), ("n_rows", C.c_int32)]


class AaeLowRank(C.Structure):
    _fields_ = [("vt_dev", C.c_void_p), ("ld", C.c_int64), ("n_features", C.c_int32), ("dims", C.c_int32)]


class AaeIrganNet(C.Structure):
    _fields_ = [("user_emb_dev", C.c_void_p), ("item_emb_dev", C.c_void_p), ("item_bias_dev", C.c_void_p),
                ("m_user_emb_dev", C.c_void_p), ("m_item_emb_dev", C.c_void_p), ("m_item_bias_dev", C.c_void_p),
                ("users", C.c_int32), ("items", C.c_int32), ("dim", C.c_int32)]


_PROTOS = {
    "aae_abi_version": (C.c_int, []),
    "aae_set_option": (C.c_int, [C.c_char_p, C.c_char_p]),
    "aae_last_error": (C.c_char_p, []),
    "aae_arena_bytes": (C.c_int, [C.POINTER(AaeConfig), C.POINTER(C.c_size_t)]),
    "aae_create": (C.c_int, [C.POINTER(AaeConfig), C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_void_p)]),
    "aae_destroy": (C.c_int, [C.c_void_p]),
    "aae_tensor_info": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(AaeTensor)]),
    "aae_set_lr": (C.c_int, [C.c_void_p, C.c_double, C.c_double]),
    "aae_params_changed": (C.c_int, [C.c_void_p]),
    "aae_set_rng_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64]),
    "aae_sync": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aae_load_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aae_store_linear": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]),
    "aae_load_adam": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]),
    "aae_store_adam": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "aae_step": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.POINTER(AaeRngInject), C.c_void_p]),
    "aae_ae_encode": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.POINTER(AaeRngInject), C.c_void_p, C.c_void_p]),
    "aae_ae_decode_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AaeRngInject), C.c_void_p, C.c_void_p]),
    "aae_vae_step": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_vae_predict": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                  C.c_void_p]),
    "aae_vae_encode": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "aae_vae_decode_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "aae_vae_encoder_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_decoder_step": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_int64, C.POINTER(AaeRngInject),
                                   C.c_void_p, C.c_void_p]),
    "aae_ae_encoder_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_disc_gen": (C.c_int, [C.c_void_p, C.POINTER(AaeRngInject), C.c_void_p]),
    "aae_disc_step": (C.c_int, [C.c_void_p, C.POINTER(AaeRngInject), C.c_void_p]),
    "aae_gen_step": (C.c_int, [C.c_void_p, C.POINTER(AaeRngInject), C.c_void_p]),
    "aae_read_losses": (C.c_int, [C.c_void_p, C.POINTER(C.c_float * 3), C.c_void_p]),
    "aae_predict": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_predict_topk": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_rank_max_rows": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "aae_rank_long_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "aae_predict_ranks": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.POINTER(AaeBatch), C.c_int32, C.c_void_p, C.c_void_p]),
    "aae_decode_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    "aae_rank_full_max_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "aae_decode_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AaeBatch), C.c_int32, C.c_int32, C.c_void_p,
                                  C.c_void_p, C.c_void_p]),
    "aae_vae_predict_topk": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p]),
    "aae_vae_predict_ranks": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p, C.POINTER(AaeBatch), C.c_int32,
                                        C.c_void_p, C.c_void_p]),
    "aae_vae_decode_topk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AaeBatch), C.c_int32, C.c_int32, C.c_void_p,
                                      C.c_void_p, C.c_void_p]),
    "aae_vae_decode_ranks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_int32,
                                       C.c_void_p, C.c_void_p]),
    "aae_vae_rank_max_rows": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int32)]),
    "aae_vae_rank_full_max_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "aae_predict_loss": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p]),
    "aae_decode_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_void_p, C.c_void_p]),
    "aae_vae_predict_loss": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AaeBatch),
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_vae_decode_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_void_p,
                                      C.c_void_p]),
    "aae_loss_max_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "aae_vae_loss_max_rows": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "aae_encode": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p]),
    "aae_decode": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_apply_updates": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "aae_apply_updates_except": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p]),
    "aae_apply_shard": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]),
    "aae_w1_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "aae_w1_packet_floats": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "aae_w1_import": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int64, C.c_int, C.c_void_p]),
    "aae_set_grad_scale": (C.c_int, [C.c_void_p, C.c_float]),
    "aae_ae_forward": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.POINTER(AaeRngInject), C.c_void_p]),
    "aae_output_layer_step": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p]),
    "aae_ae_backward": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_set_doc_l1": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aae_set_first_layer_external": (C.c_int, [C.c_void_p, C.c_int]),
    "aae_first_layer_forward": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p]),
    "aae_first_layer_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int, C.c_void_p]),
    "aae_apply_gathered": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_void_p]),
    "aae_cat_encode": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                 C.c_int64, C.c_void_p]),
    "aae_cat_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                 C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int64, C.c_void_p]),
    "aae_bag_encode": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_bag_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                 C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int64,
                                 C.c_void_p]),
    "aae_bag_update_flags": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int64,
                                       C.c_int32, C.c_void_p]),
    "aae_bag_renorm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32,
                                 C.c_void_p]),
    "aae_bag_csr_renorm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p,
                                     C.c_int64, C.c_int32, C.c_int64, C.c_double, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_bag_csr_update_flags": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64,
                                           C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int64, C.c_int32,
                                           C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_bag_csr_scratch_bytes": (C.c_int, [C.c_int64, C.c_int64, C.POINTER(C.c_int64)]),
    "aae_bag_csr_encode": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                     C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p,
                                     C.c_int64, C.c_void_p]),
    "aae_bag_csr_update": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int32, C.c_int64, C.c_int32,
                                     C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_double, C.c_int64, C.c_void_p, C.c_int64,
                                     C.c_void_p]),
    "aae_csr_embed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int64,
                                C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_cond_gather": (C.c_int, [C.POINTER(AaeCondSrc), C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int64,
                                  C.c_void_p]),
    "aae_cooc_scores": (C.c_int, [C.POINTER(AaeCooc), C.c_int32, C.POINTER(AaeBatch), C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_cooc_topk": (C.c_int, [C.POINTER(AaeCooc), C.c_int32, C.POINTER(AaeBatch), C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_cooc_ranks": (C.c_int, [C.POINTER(AaeCooc), C.c_int32, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_int32, C.c_void_p,
                                 C.c_int64, C.c_void_p, C.c_void_p]),
    "aae_cooc_scores_i32": (C.c_int, [C.POINTER(AaeCooc), C.c_int32, C.POINTER(AaeBatch), C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_cooc_topk_i32": (C.c_int, [C.POINTER(AaeCooc), C.c_int32, C.POINTER(AaeBatch), C.c_int32, C.c_int32, C.c_void_p, C.c_int64,
                                    C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_cooc_ranks_i32": (C.c_int, [C.POINTER(AaeCooc), C.c_int32, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_int32, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_void_p]),
    "aae_spgemm_i32_bound": (C.c_int, [C.POINTER(AaeCooc), C.POINTER(AaeCooc), C.c_int32, C.c_void_p, C.c_void_p]),
    "aae_spgemm_i32_count": (C.c_int, [C.POINTER(AaeCooc), C.POINTER(AaeCooc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_spgemm_i32_fill": (C.c_int, [C.POINTER(AaeCooc), C.POINTER(AaeCooc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "aae_csr_transpose_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "aae_csr_transpose_fill": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p]),
    "aae_mi_i32_marginals": (C.c_int, [C.POINTER(AaeCooc), C.POINTER(AaeCooc), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "aae_mi_i32_rows": (C.c_int, [C.POINTER(AaeCooc), C.POINTER(AaeCooc), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_void_p]),
    "aae_mi_i32_finish": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_pop_counts": (C.c_int, [C.POINTER(AaeCooc), C.c_int32, C.c_void_p, C.c_void_p]),
    "aae_pop_topk": (C.c_int, [C.POINTER(AaePopular), C.POINTER(AaeBatch), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_pop_ranks": (C.c_int, [C.POINTER(AaePopular), C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_int32, C.c_void_p, C.c_void_p]),
    "aae_rand_scores": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_rand_topk": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(AaeBatch), C.c_int32, C.c_int32, C.c_void_p,
                                C.c_void_p, C.c_void_p]),
    "aae_rand_ranks": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_int32,
                                 C.c_void_p, C.c_void_p]),
    "aae_metric_rows": (C.c_int, [C.POINTER(AaeRankRows), C.POINTER(AaeMetricSpec), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                  C.c_int64, C.c_void_p]),
    "aae_metric_finish": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "aae_ranks_from_lists": (C.c_int, [C.c_void_p, C.c_int64, C.c_int32, C.POINTER(AaeBatch), C.c_void_p, C.c_void_p]),
    "aae_spmm_f32": (C.c_int, [C.POINTER(AaeBatch), C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_lowrank_scores": (C.c_int, [C.POINTER(AaeLowRank), C.c_int32, C.POINTER(AaeBatch), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                     C.c_void_p]),
    "aae_lowrank_topk": (C.c_int, [C.POINTER(AaeLowRank), C.c_int32, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_int32, C.c_int32,
                                   C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_lowrank_ranks": (C.c_int, [C.POINTER(AaeLowRank), C.c_int32, C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.POINTER(AaeBatch),
                                    C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "aae_irgan_scratch_bytes": (C.c_int, [C.POINTER(AaeIrganNet), C.POINTER(C.c_size_t)]),
    "aae_irgan_scores": (C.c_int, [C.POINTER(AaeIrganNet), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "aae_irgan_topk": (C.c_int, [C.POINTER(AaeIrganNet), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AaeBatch), C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "aae_irgan_ranks": (C.c_int, [C.POINTER(AaeIrganNet), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(AaeBatch), C.POINTER(AaeBatch),
                                  C.c_int32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "aae_irgan_d_steps": (C.c_int, [C.POINTER(AaeIrganNet), C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aae_irgan_sample_neg": (C.c_int, [C.POINTER(AaeIrganNet), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_uint64,
                                       C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aae_irgan_g_steps": (C.c_int, [C.POINTER(AaeIrganNet), C.POINTER(AaeIrganNet), C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int64, C.c_float, C.c_float, C.c_void_p,
                                    C.c_void_p, C.c_size_t, C.c_void_p]),
    "aae_dense_to_csr": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int64, C.c_void_p, C.POINTER(C.c_int32 * 4), C.c_void_p]),
    "aae_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
    "aae_profile_read": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "aae_join": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aae_join_output_layer": (C.c_int, [C.c_void_p, C.c_void_p]),
    "aae_rccl_unique_id": (C.c_int, [C.c_char_p]),
    "aae_rccl_init": (C.c_int, [C.c_char_p, C.c_int32, C.c_int32, C.POINTER(AaeCollectives)]),
    "aae_rccl_destroy": (C.c_int, [C.POINTER(AaeCollectives)]),
    "aae_dp_step": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(AaeCollectives), C.POINTER(AaeBatch), C.POINTER(AaeBatch),
                              C.POINTER(AaeBatch), C.c_void_p, C.POINTER(AaeRngInject), C.c_void_p]),
    "aae_dp_reserve": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32]),
    "aae_shard_step": (C.c_int, [C.c_void_p, C.POINTER(AaeCollectives), C.POINTER(AaeBatch), C.POINTER(AaeBatch), C.c_void_p,
                                 C.POINTER(AaeRngInject), C.c_float, C.c_void_p]),
    "aae_memcpy_sync": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "aae_echo_collectives": (C.c_int, [C.c_int32, C.POINTER(AaeCollectives)]),
    "aae_ipc_create": (C.c_int, [C.c_int64, C.c_char_p, C.POINTER(C.c_void_p)]),
    "aae_ipc_init": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int32, C.c_int32, C.c_int64, C.POINTER(AaeCollectives)]),
    "aae_ipc_destroy": (C.c_int, [C.POINTER(AaeCollectives), C.c_void_p]),
    "aae_set_input_noise": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64]),
    "aae_set_input_noise_gen": (C.c_int, [C.c_void_p, C.c_float]),
    "aae_dae_thin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p]),
    "aae_prefetch_batch": (C.c_int, [C.c_void_p, C.POINTER(AaeBatch)]),
    "aae_set_split": (C.c_int, [C.c_void_p, C.c_int32]),
}
K_ENC_GATHER, K_DEC_BCE_FWD, K_DEC_DA2, K_DEC_DV3_ADAM, K_ENC_W1_ADAM, K_DEC_FUSED, K_CHAIN, K_DEC_CRIT, K_DEC_OPT, K_RANK, K_COLLECTIVE = range(11)
K_UNIQ_ITEMS, K_W1_CATCHUP = 11, 12
K_VAE_REPARAM = 13        # the reparametrisation kernels of a VAE handle on the per-layer route (csrc/vae_layers.h)

_lib = None


class AaeHipError(RuntimeError):
    pass


def _destroy_handle(lib, handle, arena, pid):
    # (a fork()ed child - e.g. a multiprocessing.Manager server started by the process that owns the model - inherits
    # the Python object but not a usable HIP runtime: only the creating process talks to the library)
    if os.getpid() == pid:
        try:
            lib.aae_destroy(handle)
        except Exception:
            pass
    del arena


def load_library():
    """dlopen the library and bind every symbol of the header.  Raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  There is no CPU fallback for the AAE step.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _PROTOS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype, fn.argtypes = res, args
    if lib.aae_abi_version() != ABI_VERSION:
        raise ImportError("libaaerec_hip.so ABI version mismatch")
    _lib = lib
    return lib


def set_option(name, value):
    """A switch of the library for the handles created from now on (aae_set_option; names: struct aae_options,
    csrc/abi_model.h - e.g. 'RANK_COLLECT_CAP', the entries of a row's collect list in the k > 32 ranking path).
    value None hands the name back to the environment variable AAE_<name>."""
    _check(load_library().aae_set_option(str(name).encode(), None if value is None else str(value).encode()))


def _check(rc):
    if rc != 0:
        raise AaeHipError(f"libaaerec_hip error {rc}: {load_library().aae_last_error().decode()}")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _arg(a):
    """An argument of an entry point: a device tensor (None: absent) by its address, a struct by reference, anything else as
    it is.  The caller's argument tuple keeps every tensor alive until the call is enqueued."""
    if a is None or torch.is_tensor(a):
        return _ptr(a)
    return C.byref(a) if isinstance(a, C.Structure) else a


_UPLOAD_STREAMS = {}


def upload(x, device, dtype=None):
    """Host -> HBM copy of a small per-batch operand (condition inputs, index blocks) that does not drain the queue.

    A blocking copy from pageable memory on the compute stream waits for every kernel already enqueued there, so a
    training loop that uploads something per batch runs host and GPU in lock-step.  The copy goes through a side
    stream instead: the host waits for the copy alone, and because it has completed before this function returns,
    whatever is enqueued afterwards on the compute stream sees the data.  Device tensors pass through."""
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    dev = torch.device(device)
    if t.is_cuda or dev.type != "cuda":
        return t.to(dev, dtype) if dtype is not None else t.to(dev)
    if dtype is not None:
        t = t.to(dtype)
    side = _UPLOAD_STREAMS.get(dev)
    if side is None:
        side = _UPLOAD_STREAMS[dev] = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        out = t.to(dev)
    out.record_stream(torch.cuda.current_stream(dev))
    return out


class HostRows:
    """The [n_rows, n_cols] float32 host matrix a predict loop hands back (the reference's predict() returns the
    dense score matrix, aae.py:840-870), filled batch by batch.  The matrix is allocated once in page-locked memory
    and each device batch is copied straight into its rows asynchronously - 56 GB/s on the MI355X host link against
    5 GB/s for batch.cpu().numpy() + np.vstack (three passes over pageable memory).  Above PIN_LIMIT bytes, or if
    pinning fails, the same scheme runs on a pageable matrix."""
    PIN_LIMIT = 32 << 30

    def __init__(self, n_rows, n_cols, device):
        self.device = torch.device(device)
        self.pinned = n_rows * n_cols * 4 <= self.PIN_LIMIT
        if self.pinned:
            try:
                self.host = torch.empty(n_rows, n_cols, dtype=torch.float32, pin_memory=True)
            except RuntimeError:
                self.pinned = False
        if not self.pinned:
            self.host = torch.empty(n_rows, n_cols, dtype=torch.float32)

    def put(self, start, batch):
        self.host[start:start + batch.shape[0]].copy_(batch, non_blocking=self.pinned)

    def numpy(self):
        if self.pinned:
            torch.cuda.current_stream(self.device).synchronize()
        return self.host.numpy()


def _cond_operands(table, block, source, state=()):
    """Operand checks of the condition kernels (shapes must match what the kernels index): the table, the [rows, dim] block
    (an encode's out, an update's dout; None: a renorm has none), the source - a padded idx block or a BagWindow - and an
    update's moments and gradient scratch."""
    idx = None if isinstance(source, BagWindow) else source
    rows = source.rows if idx is None else idx.shape[0]
    if not (table.is_cuda and (block is None or block.is_cuda) and (source.bags.indptr if idx is None else idx).is_cuda):
        raise RuntimeError("aaerec: the condition kernels take GPU tensors (there is no CPU path)")
    if table.dtype != torch.float32 or not table.is_contiguous() or table.dim() != 2:
        raise TypeError("aaerec: embedding table must be a contiguous float32 [vocab, dim] tensor")
    if idx is not None and (idx.dtype != torch.int32 or idx.dim() != 2 or not idx.is_contiguous()):
        raise TypeError("aaerec: idx must be a contiguous int32 [rows, width] tensor")
    if block is not None and (block.dtype != torch.float32 or block.dim() != 2 or block.stride(1) != 1
                              or block.shape[0] != rows or block.shape[1] != table.shape[1]):
        raise TypeError("aaerec: block must be a float32 [rows, dim] view with unit column stride")
    for t in state[:2] + tuple(t for t in state[2:] if t is not None):          # (the gradient scratch may be absent)
        if t.shape != table.shape or t.dtype != torch.float32 or not t.is_contiguous() or t.device != table.device:
            raise TypeError("aaerec: optimiser state must match the embedding table")


def _cond_call(entry, table, *args):
    """entry(table, *args, stream) on the table's device and current stream; a tensor (None: absent) goes by its address.
    (Twice a step on a host-bound path: one inline test per argument, not _arg, which measured 4-7 us a call more.)"""
    args = [_ptr(a) if a is None or isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(table.device):
        _check(entry(_ptr(table), *args, _stream_of(table.device)))


def cat_encode(table, idx, out, mean=False):
    """CategoricalCondition.encode on the device: out[r] = sum (or mean over the padded width) of table[idx[r, w]];
    index 0 reads as zero.  `out` may be a column slice of the step's condition block."""
    _cond_operands(table, out, idx)
    _cond_call(load_library().aae_cat_encode, table, table.shape[0], table.shape[1], idx, idx.shape[0], idx.shape[1],
               CAT_MEAN if mean else CAT_SUM, out, out.stride(0))


def cat_update(table, exp_avg, exp_avg_sq, idx, dout, lr, step, mean=False, grad_scratch=None):
    """Backward of cat_encode from dout [rows, dim] plus the condition's optimiser step: SparseAdam over the rows the
    batch names, or (grad_scratch given: zeros [vocab, dim]) dense Adam over the whole table.  step counts from 1."""
    _cond_operands(table, dout, idx, (exp_avg, exp_avg_sq, grad_scratch))
    _cond_call(load_library().aae_cat_update, table, exp_avg, exp_avg_sq, grad_scratch, table.shape[0], table.shape[1], idx,
               idx.shape[0], idx.shape[1], CAT_MEAN if mean else CAT_SUM, dout, dout.stride(0),
               CAT_ADAM if grad_scratch is not None else CAT_SPARSE_ADAM, float(lr), int(step))


def bag_encode(table, idx, out, reduce=BAG_SUM, padding_idx=-1):
    """A bag of table rows per row of idx, reduced into out [rows, dim] (aae_bag_encode: nn.EmbeddingBag's sum / mean / max
    and CategoricalCondition's hid.sum(1) / .mean(1) / .max(1)[0]).  reduce: one of BAG_*; padding_idx -1: no padding row.
    `out` may be a column slice of the step's condition block."""
    _cond_operands(table, out, idx)
    _cond_call(load_library().aae_bag_encode, table, table.shape[0], table.shape[1], idx, idx.shape[0], idx.shape[1],
               int(reduce), int(padding_idx), out, out.stride(0))


def bag_update(table, exp_avg, exp_avg_sq, idx, dout, lr, step, reduce=BAG_SUM, padding_idx=-1, grad_scratch=None,
               sparse=False, scale_by_freq=False):
    """Backward of bag_encode from dout [rows, dim] plus the optimiser step: dense Adam over the whole table, or
    (sparse=True) SparseAdam over the rows the batch names.  grad_scratch (zeros [vocab, dim], left zero): needed by dense
    Adam and by the two max modes.  The winners of the max modes are recomputed from the table: it must be what bag_encode
    read.  step counts from 1.  scale_by_freq (scale_grad_by_freq; dense Adam only): a table row's gradient is divided by
    the number of times the block names it."""
    _cond_operands(table, dout, idx, (exp_avg, exp_avg_sq, grad_scratch))
    _cond_call(load_library().aae_bag_update_flags, table, exp_avg, exp_avg_sq, grad_scratch, table.shape[0], table.shape[1], idx,
               idx.shape[0], idx.shape[1], int(reduce), int(padding_idx), dout, dout.stride(0),
               CAT_SPARSE_ADAM if sparse else CAT_ADAM, float(lr), int(step), BAG_SCALE_BY_FREQ if scale_by_freq else 0)


def _renorm_operands(table, source, max_norm, norm_type):
    if float(norm_type) not in BAG_NORM_TYPES:
        raise ValueError("aaerec: the renorm kernels take norm_type 1, 2 or inf")
    _cond_operands(table, None, source)
    return float(max_norm), BAG_NORM_TYPES[float(norm_type)]


def bag_renorm(table, idx, max_norm, norm_type=2.0):
    """nn.Embedding's max_norm on the device (aae_bag_renorm), in front of bag_encode: every distinct table row idx names - a
    padding row too - whose norm_type-norm exceeds max_norm is scaled onto it, once."""
    max_norm, code = _renorm_operands(table, idx, max_norm, norm_type)
    _cond_call(load_library().aae_bag_renorm, table, table.shape[0], table.shape[1], idx, idx.shape[0], idx.shape[1], max_norm, code)


# ---- bags from a resident CSR (aae_bag_csr_*; csrc/cond_csr.h) -------------------------------------------------------
BAG_CSR_SORT = 4096              # kBagCsrSort: keys one workgroup sorts in LDS, the run length the merge passes start from
BAG_CSR_SCAN = 1024              # kBagCsrScanNT: rows the row scan takes in one round
BAG_CSR_UPDATE_WAVES = 4096 * 4  # kBagCsrMaxGrid * kCatWaves: sorted positions the update launch takes in one grid round
BAG_CSR_MAX_ENTRIES = 1 << 22    # kBagCsrMaxEntries: entries of a step


def bag_csr_scratch_bytes(max_rows, max_entries):
    """Bytes of the scratch a step of max_rows rows and at most max_entries entries needs (arithmetic: no GPU)."""
    n = C.c_int64()
    _check(load_library().aae_bag_csr_scratch_bytes(int(max_rows), int(max_entries), C.byref(n)))
    return n.value


def bags_from_lists(lists):
    """(indptr int64 [n + 1], indices int32) of a list of value lists, entry order kept.  A value that does not fit an int32
    names no table row: it becomes -1, which every reduction skips."""
    lens = np.fromiter((len(row) for row in lists), dtype=np.int64, count=len(lists))
    indptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum(lens, out=indptr[1:])
    flat = np.fromiter((v for row in lists for v in row), dtype=np.int64, count=int(indptr[-1]))
    return indptr, _bag_ids(flat)


def _bag_ids(flat):
    flat = np.asarray(flat, dtype=np.int64)
    return np.where((flat < -2 ** 31) | (flat >= 2 ** 31), -1, flat).astype(np.int32)


def bags_from_offsets(indices, offsets, weights=None, include_last_offset=False):
    """(indptr, indices, weights) of nn.EmbeddingBag's 1-D call form: bag i holds indices[offsets[i]:offsets[i + 1]], the
    last one runs to the end - or, include_last_offset, offsets already ends with len(indices)."""
    indices = np.asarray(indices).reshape(-1)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1)
    indptr = offsets if include_last_offset else np.concatenate([offsets, [len(indices)]]).astype(np.int64)
    if len(indptr) < 1 or (len(indptr) > 1 and indptr[0] != 0) or (np.diff(indptr) < 0).any() or indptr[-1] > len(indices):
        raise ValueError("aaerec: offsets must start at 0, ascend and stay within the indices")
    if weights is not None:
        weights = np.asarray(weights, dtype=np.float32).reshape(-1)
        if len(weights) != len(indices):
            raise ValueError("aaerec: per_sample_weights must have the shape of the indices")
    return np.ascontiguousarray(indptr), _bag_ids(indices), weights


class DeviceBags:
    """The value lists of a whole corpus as a CSR resident in HBM (int64 indptr, int32 indices - table rows, in list order,
    repeats kept -, optionally float32 per-sample weights), uploaded once.  `lengths` (device int32) holds the lists'
    lengths; entry_bound(rows) bounds the entries of any `rows` lists from the host's sorted copy, so a step needs no
    synchronisation to size its scratch.  window() names the rows of a step."""

    def __init__(self, lists, device, weights=None):
        indptr, indices = bags_from_lists(lists)
        self._init(indptr, indices, None if weights is None else np.asarray(weights, dtype=np.float32).reshape(-1), device)

    @classmethod
    def from_offsets(cls, indices, offsets, device, weights=None, include_last_offset=False):
        self = cls.__new__(cls)
        self._init(*bags_from_offsets(indices, offsets, weights, include_last_offset), device)
        return self

    def _init(self, indptr, indices, weights, device):
        self.device = torch.device(device)
        self.n_docs, self.nnz = len(indptr) - 1, int(indptr[-1])
        if weights is not None and len(weights) != len(indices):
            raise ValueError("aaerec: per_sample_weights must have the shape of the indices")
        lens = np.diff(indptr)
        self._cum = np.cumsum(np.sort(lens)[::-1])           # _cum[k - 1]: the entries of the k longest lists
        self.indptr = upload(indptr, device)
        self.indices = upload(indices if len(indices) else np.zeros(1, dtype=np.int32), device)
        self.weights = None if weights is None else upload(weights if len(weights) else np.zeros(1, dtype=np.float32), device)
        self.lengths = upload(lens.astype(np.int32), device)
        self.device = self.indptr.device                     # ('cuda' resolved to the device the arrays went to)
        self._scratch = None

    def __len__(self):
        return self.n_docs

    def entry_bound(self, rows):
        """No `rows` lists of the corpus hold more entries than this (at least 1)."""
        if self.n_docs == 0 or rows < 1:
            return 1
        return max(1, int(self._cum[min(int(rows), self.n_docs) - 1]))

    def scratch(self, rows):
        """(buffer, bytes) for a step of `rows` rows: grown when a call needs more, never per step."""
        need = bag_csr_scratch_bytes(rows, self.entry_bound(rows))
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self._scratch, self._scratch.numel()

    def window(self, row_ids=None, row0=0, rows=None):
        """The rows of a step: a device int32 tensor of row ids (a window of the epoch's permutation), or the contiguous
        rows row0 .. row0 + rows."""
        return BagWindow(self, row_ids, int(row0), int(row_ids.numel() if row_ids is not None else rows))


class BagWindow:
    """(DeviceBags, rows of a step): what a resident condition's encode_into / update_from take instead of value lists."""
    __slots__ = ("bags", "row_ids", "row0", "rows")

    def __init__(self, bags, row_ids, row0, rows):
        if row_ids is not None and (row_ids.dtype != torch.int32 or row_ids.dim() != 1 or not row_ids.is_contiguous()
                                    or row_ids.device != bags.device):
            raise TypeError("aaerec: row_ids must be a contiguous int32 vector on the bags' device")
        self.bags, self.row_ids, self.row0, self.rows = bags, row_ids, row0, rows

    def __len__(self):
        return self.rows


def bag_csr_encode(table, view, out, reduce=BAG_SUM, padding_idx=-1):
    """bag_encode over the rows `view` (a BagWindow) of a resident DeviceBags: the same bits as bag_encode / cat_encode on
    those lists padded to their longest.  `out` may be a column slice of the step's condition block."""
    b = view.bags
    _cond_operands(table, out, view)
    scratch, nbytes = b.scratch(view.rows)
    _cond_call(load_library().aae_bag_csr_encode, table, table.shape[0], table.shape[1], b.indptr, b.indices, b.weights,
               b.n_docs, b.nnz, view.row_ids, view.row0, view.rows, int(reduce), int(padding_idx), out, out.stride(0), scratch, nbytes)


def bag_csr_update(table, exp_avg, exp_avg_sq, view, dout, lr, step, reduce=BAG_SUM, padding_idx=-1, grad_scratch=None,
                   sparse=False, scale_by_freq=False):
    """bag_update over the rows `view` of a resident DeviceBags: entries grouped by table row with a sort (no quadratic scan,
    nothing on the host), summed in the padded route's order - the same bits.  Arguments as bag_update."""
    b = view.bags
    _cond_operands(table, dout, view, (exp_avg, exp_avg_sq, grad_scratch))
    scratch, nbytes = b.scratch(view.rows)
    _cond_call(load_library().aae_bag_csr_update_flags, table, exp_avg, exp_avg_sq, grad_scratch, table.shape[0], table.shape[1],
               b.indptr, b.indices, b.weights, b.n_docs, b.nnz, view.row_ids, view.row0, view.rows, b.entry_bound(view.rows),
               int(reduce), int(padding_idx), dout, dout.stride(0), CAT_SPARSE_ADAM if sparse else CAT_ADAM, float(lr), int(step),
               BAG_SCALE_BY_FREQ if scale_by_freq else 0, scratch, nbytes)


def bag_csr_renorm(table, view, max_norm, norm_type=2.0):
    """bag_renorm over the rows `view` of a resident DeviceBags (aae_bag_csr_renorm): the same bits as on those lists padded."""
    b = view.bags
    max_norm, code = _renorm_operands(table, view, max_norm, norm_type)
    scratch, nbytes = b.scratch(view.rows)
    _cond_call(load_library().aae_bag_csr_renorm, table, table.shape[0], table.shape[1], b.indptr, b.indices, b.n_docs, b.nnz,
               view.row_ids, view.row0, view.rows, b.entry_bound(view.rows), max_norm, code, scratch, nbytes)


# ---- constant condition blocks resident in HBM (aae_cond_gather; csrc/cond_gather.h) -----------------------------------
COND_SRC_MAX = 8                 # AAE_COND_SRC_MAX: blocks of one aae_cond_gather call


class DeviceBlock:
    """The dense counterpart of DeviceBags: the [n_docs, width] float32 matrix of a constant condition (the document vectors
    of a PretrainedWordEmbeddingCondition) resident in HBM - uploaded once, or wrapped around a CUDA tensor without a copy.
    window() names the rows of a step; cond_gather copies the windows of up to COND_SRC_MAX blocks into a condition block."""

    def __init__(self, data, device=None):
        if torch.is_tensor(data) and data.is_cuda:
            if data.dtype != torch.float32 or data.dim() != 2 or (data.shape[1] > 1 and data.stride(1) != 1) or data.stride(0) < data.shape[1]:
                raise TypeError("aaerec: a resident condition block is a float32 [n_docs, width] tensor with unit column stride")
            self.data = data
        else:
            if np.ndim(data) != 2:
                raise TypeError("aaerec: a resident condition block is a [n_docs, width] matrix")
            if device is None:
                raise ValueError("aaerec: DeviceBlock of host data needs the device to upload it to")
            self.data = upload(data, device, torch.float32)
        if self.data.shape[1] < 1:
            raise ValueError("aaerec: a resident condition block has at least one column")
        self.device = self.data.device
        self.n_docs, self.width = int(self.data.shape[0]), int(self.data.shape[1])

    def __len__(self):
        return self.n_docs

    def window(self, row_ids=None, row0=0, rows=None):
        """The rows of a step, named as DeviceBags.window names them: a device int32 tensor of row ids (a window of the
        epoch's permutation), or the contiguous rows row0 .. row0 + rows."""
        return BlockWindow(self, row_ids, int(row0), int(row_ids.numel() if row_ids is not None else rows))


class BlockWindow:
    """(DeviceBlock, rows of a step): what cond_gather takes."""
    __slots__ = ("block", "row_ids", "row0", "rows")

    def __init__(self, block, row_ids, row0, rows):
        if row_ids is not None and (row_ids.dtype != torch.int32 or row_ids.dim() != 1 or not row_ids.is_contiguous()
                                    or row_ids.device != block.device):
            raise TypeError("aaerec: row_ids must be a contiguous int32 vector on the block's device")
        self.block, self.row_ids, self.row0, self.rows = block, row_ids, row0, rows

    def __len__(self):
        return self.rows


def _cond_col0s(widths, col0s):
    if col0s is None:
        return [int(c) for c in np.cumsum([0] + list(widths[:-1]))]
    if len(col0s) != len(widths):
        raise ValueError("aaerec: cond_gather takes one col0 per window")
    return [int(c) for c in col0s]


def cond_gather(windows, out=None, col0s=None):
    """The rows the windows name - BlockWindows of up to COND_SRC_MAX DeviceBlocks, all naming the SAME rows - copied into
    `out` [rows, >= the columns named] at the column offsets col0s (None: one block behind the other from column 0), in one
    launch (aae_cond_gather).  out None: a new [rows, sum of the widths] tensor.  Columns no window names keep their content;
    a row id outside a block gives a row of zeros.  Returns out."""
    windows = list(windows)
    if not 1 <= len(windows) <= COND_SRC_MAX:
        raise ValueError("aaerec: cond_gather takes 1 to %d windows" % COND_SRC_MAX)
    w0 = windows[0]
    for w in windows[1:]:
        if w.rows != w0.rows or w.row0 != w0.row0 or (w.row_ids is None) != (w0.row_ids is None) or \
                (w.row_ids is not None and w.row_ids.data_ptr() != w0.row_ids.data_ptr()) or w.block.device != w0.block.device:
            raise ValueError("aaerec: the windows of one cond_gather name the same rows on one device")
    col0s = _cond_col0s([w.block.width for w in windows], col0s)
    dev = w0.block.device
    if out is None:
        out = torch.empty(w0.rows, max(c + w.block.width for c, w in zip(col0s, windows)), dtype=torch.float32, device=dev)
    if out.dtype != torch.float32 or out.dim() != 2 or out.device != dev or out.shape[0] != w0.rows or \
            (out.shape[1] > 1 and out.stride(1) != 1):
        raise TypeError("aaerec: out must be a float32 [rows, columns] view with unit column stride on the blocks' device")
    if any(c < 0 or c + w.block.width > out.shape[1] for c, w in zip(col0s, windows)):
        raise ValueError("aaerec: a window's columns lie outside out")
    srcs = (AaeCondSrc * len(windows))(*(AaeCondSrc(w.block.data.data_ptr(), w.block.data.stride(0), w.block.n_docs,
                                                    w.block.width, c) for c, w in zip(col0s, windows)))
    with torch.cuda.device(dev):
        _check(load_library().aae_cond_gather(srcs, len(windows), _ptr(w0.row_ids), w0.row0, w0.rows, _ptr(out),
                                              out.stride(0) if w0.rows > 1 else max(out.stride(0), out.shape[1]), _stream_of(dev)))
    return out


def cond_gather_host(tables, row_ids=None, row0=0, rows=None, out=None, col0s=None):
    """cond_gather restated in NumPy (the tests' oracle): tables are float32 [n_docs, width] arrays (any row stride), row_ids
    an integer vector or None for row0 .. row0 + rows, out a float32 [rows, columns] array (None: a new one of zeros, as wide
    as the columns named).  Words move as uint32, so every bit arrives."""
    tables = [np.asarray(t) for t in tables]
    if any(t.dtype != np.float32 or t.ndim != 2 for t in tables):
        raise TypeError("aaerec: cond_gather_host takes float32 [n_docs, width] arrays")
    ids = np.arange(row0, row0 + rows, dtype=np.int64) if row_ids is None else np.asarray(row_ids, dtype=np.int64).reshape(-1)
    col0s = _cond_col0s([t.shape[1] for t in tables], col0s)
    if out is None:
        out = np.zeros((len(ids), max(c + t.shape[1] for c, t in zip(col0s, tables))), dtype=np.float32)
    bits = out.view(np.uint32)
    for c, t in zip(col0s, tables):
        live = (ids >= 0) & (ids < t.shape[0])
        part = np.zeros((len(ids), t.shape[1]), dtype=np.uint32)
        if live.any():
            part[live] = np.ascontiguousarray(t[ids[live]]).view(np.uint32)
        bits[:, c:c + t.shape[1]] = part
    return out


def csr_embed(csr, table, out=None):
    """[rows, dim] device tensor: row r = sum of csr.values[e] * table[csr.indices[e]] over the entries of row r
    (EmbeddedVectorizer.transform's `sparse_scores @ embedding`, reference ub.py:52-57).  out: a float32 [rows, dim] view
    with unit column stride on the table's device to write into (rows of a larger matrix); None: a new tensor."""
    if not table.is_cuda or table.dtype != torch.float32 or table.dim() != 2 or table.stride(1) != 1:
        raise TypeError("aaerec: table must be a float32 [vocab, dim] GPU tensor with unit column stride")
    if csr.shape[1] > table.shape[0]:
        raise ValueError("aaerec: the sparse matrix has more columns than the table has rows")
    if out is None:
        out = torch.empty(csr.shape[0], table.shape[1], dtype=torch.float32, device=table.device)
    elif out.dtype != torch.float32 or out.device != table.device or tuple(out.shape) != (csr.shape[0], table.shape[1]) \
            or (out.shape[1] > 1 and out.stride(1) != 1) or (out.shape[0] > 1 and out.stride(0) < out.shape[1]):
        raise TypeError("aaerec: out must be a float32 [rows, dim] view with unit column stride on the table's device")
    with torch.cuda.device(table.device):
        _check(load_library().aae_csr_embed(_ptr(csr.indptr), _ptr(csr.indices), _ptr(csr.values), csr.shape[0],
                                            _ptr(table), table.shape[0], table.shape[1], table.stride(0), _ptr(out),
                                            out.stride(0),
                                            C.c_void_p(torch.cuda.current_stream(table.device).cuda_stream)))
    return out


_GENERATION = itertools.count(1)


def row_ids(rows, generation):
    """Tag a device int32 row-id tensor with the caller's content id (aae_batch.generation, ABI 3): the same id for every
    view of one buffer while its content stands, a new one after any rewrite or re-allocation.  A batch whose row ids carry
    no tag is never matched with work built ahead for it (aae_prefetch_batch): a slice of a tensor is a new Python object at
    an address the allocator may have handed out before, and nothing but the caller knows whether the ids in it changed."""
    rows._aae_generation = int(generation)
    return rows


class DeviceCSR:
    """A CSR matrix resident in HBM (int64 indptr, int32 indices, float32 values).  `generation` names its content
    (aae_batch.generation): unique per object; call touch() after rewriting the arrays in place."""

    def touch(self):
        self.generation = next(_GENERATION)

    def __init__(self, X, device):
        X = X.tocsr()
        X.sum_duplicates()
        self.generation = next(_GENERATION)
        self.shape = X.shape
        self.nnz_per_row_max = int(np.diff(X.indptr).max()) if X.shape[0] else 0
        self.indptr = upload(X.indptr.astype(np.int64), device)
        # (a matrix without entries - e.g. an item slice none of the batch's documents touches - still hands the
        # library valid pointers: one unused element)
        self.indices = upload(X.indices.astype(np.int32) if X.nnz else np.zeros(1, dtype=np.int32), device)
        self.values = upload(X.data.astype(np.float32) if X.nnz else np.zeros(1, dtype=np.float32), device)

    @classmethod
    def from_dense(cls, X, device, capacity):
        """The reference's call form (aae.py:745-754): a dense [rows, n_cols] float32 / float64 batch.  The matrix is
        uploaded as it is (one pass of host memory: no host-side scan, no float64 -> float32 copy) and compacted on the
        device (aae_dense_to_csr); raises like the reference's BCE for values outside [0, 1]."""
        X = np.ascontiguousarray(X)
        if X.dtype not in (np.float32, np.float64):
            X = X.astype(np.float32)
        if X.ndim != 2:
            raise ValueError("expected a 2-D batch")
        dev = torch.device(device)
        rows, n_cols = X.shape
        dense = upload(X, dev)
        self = cls.__new__(cls)
        self.generation = next(_GENERATION)
        self.shape = (rows, n_cols)
        cap = int(max(1, min(int(capacity), rows * n_cols)))
        self.indptr = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        self.indices = torch.empty(cap, dtype=torch.int32, device=dev)
        self.values = torch.empty(cap, dtype=torch.float32, device=dev)
        scratch = torch.empty(rows + 8, dtype=torch.int32, device=dev)
        stats = (C.c_int32 * 4)()
        with torch.cuda.device(dev):
            _check(load_library().aae_dense_to_csr(_ptr(dense), X.dtype.itemsize, n_cols, rows, n_cols, _ptr(self.indptr),
                                                   _ptr(self.indices), _ptr(self.values), cap, _ptr(scratch), C.byref(stats),
                                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
        if stats[2]:
            raise RuntimeError("all elements of target should be between 0 and 1")
        if stats[3]:
            raise ValueError(f"the batch holds {stats[1]} entries, more than the model's capacity of {cap} (max_nnz)")
        self.nnz_per_row_max = int(stats[0])
        self.nnz = int(stats[1])
        return self

    @classmethod
    def from_arrays(cls, indptr, indices, values, n_cols, device):
        self = cls.__new__(cls)
        self.generation = next(_GENERATION)
        self.shape = (len(indptr) - 1, n_cols)
        self.nnz_per_row_max = int(np.diff(indptr).max()) if len(indptr) > 1 else 0
        self.indptr = upload(np.asarray(indptr, dtype=np.int64), device)
        self.indices = upload(np.asarray(indices, dtype=np.int32) if len(indices) else np.zeros(1, dtype=np.int32), device)
        self.values = upload(np.asarray(values, dtype=np.float32) if len(values) else np.zeros(1, dtype=np.float32), device)
        return self


# ---- the item co-occurrence baseline (aae_cooc_*; csrc/cooc.h) -----------------------------------------------------
class DeviceCooc:
    """A co-occurrence matrix resident in HBM as the kernels read it: int64 indptr, int32 indices (ascending within a
    row), int32 values.  `C` is a scipy matrix [items, items] with whole-number values below 2^31 (aaerec.cooc checks)."""

    def __init__(self, C, device):
        C = C.tocsr()
        C.sum_duplicates()
        C.sort_indices()
        self.shape = C.shape
        self.nnz = int(C.nnz)
        self.device = torch.device(device)
        self.indptr = upload(C.indptr.astype(np.int64), device)
        self.indices = upload(C.indices.astype(np.int32) if C.nnz else np.zeros(1, dtype=np.int32), device)
        self.values = upload(np.rint(C.data).astype(np.int32) if C.nnz else np.zeros(1, dtype=np.int32), device)
        self._row_abs_max = np.asarray(abs(C).max(axis=1).toarray(), dtype=np.float64).ravel() if C.nnz else np.zeros(C.shape[0])

    @classmethod
    def from_device(cls, indptr, indices, values, shape, device):
        """The matrix from device tensors as they stand - int64 indptr [rows + 1], int32 indices / values [>= max(1, nnz)], the
        columns ascending within a row: no host round trip beyond the one number nnz = indptr[-1]."""
        self = cls.__new__(cls)
        self.shape = (int(shape[0]), int(shape[1]))
        self.device = torch.device(device)
        for t, dt in ((indptr, torch.int64), (indices, torch.int32), (values, torch.int32)):
            if not t.is_cuda or t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.numel() < 1:
                raise TypeError("aaerec: from_device takes contiguous GPU vectors: int64 indptr, int32 indices, int32 values")
        if indptr.numel() != self.shape[0] + 1:
            raise ValueError("aaerec: indptr must hold rows + 1 offsets")
        self.nnz = int(indptr[-1])
        if indices.numel() < self.nnz or values.numel() < self.nnz:
            raise ValueError("aaerec: indices / values are shorter than indptr[-1]")
        self.indptr, self.indices, self.values = indptr, indices, values
        self._row_abs_max = None
        return self

    def to_scipy(self):
        """The matrix on the host: a canonical scipy CSR with int64 values."""
        import scipy.sparse as sp
        return sp.csr_matrix((self.values[:self.nnz].cpu().numpy().astype(np.int64), self.indices[:self.nnz].cpu().numpy(),
                              self.indptr.cpu().numpy()), shape=self.shape)

    def abs_max(self):
        """max |value| over the stored entries (0 without any): a device reduction, one number to the host."""
        return int(self.values[:self.nnz].abs().max()) if self.nnz else 0

    def row_abs_max(self):
        """m_i = max_j |C_ij| per row (0 for an empty one): a host array of float64 [rows], kept.  From the scipy matrix the
        object was made from; for a matrix made on the device one reduction over the CSR values there and rows numbers to the
        host - never the matrix.  (aaerec.cooc.device_route bounds a row's scores by it.)"""
        if self._row_abs_max is None:
            m = torch.zeros(self.shape[0], dtype=torch.int64, device=self.device)
            if self.nnz:
                rows = torch.repeat_interleave(torch.arange(self.shape[0], device=self.device), self.indptr.diff())
                m.scatter_reduce_(0, rows, self.values[:self.nnz].to(torch.int64).abs(), "amax")
            self._row_abs_max = m.cpu().numpy().astype(np.float64)
        return self._row_abs_max

    def struct(self):
        c = AaeCooc()
        c.indptr_dev, c.indices_dev, c.values_dev = self.indptr.data_ptr(), self.indices.data_ptr(), self.values.data_ptr()
        c.n_rows = int(self.shape[0])
        return c


def _csr_batch(csr, row_start, n_rows, rows=None):
    """The aae_batch of rows [row_start, row_start + n_rows) of a DeviceCSR (or of the rows named by `rows`) for the handle-free
    calls: no per-model bounds, no content id."""
    b = AaeBatch()
    b.indptr_dev, b.indices_dev, b.values_dev = csr.indptr.data_ptr(), csr.indices.data_ptr(), csr.values.data_ptr()
    b.rows_dev = rows.data_ptr() if rows is not None else None
    b.row_start, b.n_rows = int(row_start), int(n_rows)
    b.max_row_nnz = int(csr.nnz_per_row_max)
    b.nnz_bound = int(min(n_rows * max(1, csr.nnz_per_row_max), 2 ** 31 - 1))
    return b


def _scratch(device, n_rows, width, scratch, dtype, what, aligned):
    """[n_rows, ld] of `dtype` on `device`, ld = width rounded up to 4: the caller's (at least n_rows x width, unit column
    stride; aligned: on a 16-byte aligned base with a row stride that is a multiple of 4, what the float4 loads of the
    truncated-SVD kernels need) or a new one."""
    if scratch is None:
        return torch.empty(n_rows, (width + 3) & ~3, dtype=dtype, device=device)
    if not scratch.is_cuda or scratch.dtype != dtype or scratch.dim() != 2 or scratch.stride(1) != 1 or scratch.shape[0] < n_rows \
            or scratch.shape[1] < width or (aligned and (scratch.stride(0) % 4 or scratch.data_ptr() % 16)):
        raise TypeError("aaerec: {} must be a {}{} GPU matrix of at least [n_rows, {}] with unit column stride{}".format(
            what, "16-byte aligned " if aligned else "", "float32" if dtype == torch.float32 else "int32", width,
            " and a row stride that is a multiple of 4" if aligned else ""))
    return scratch


def _stream_of(device):
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# The two skeletons of every ranking call, a model handle's and the handle-free baselines' alike.  ctx: a context that makes
# `device` current; lead, mid: the entry point's other arguments as _arg takes them.
def _list_call(entry, device, ctx, n_rows, k, exclude_known, lead, mid=()):
    """(ids int32 [n_rows, k], scaled scores float32 [n_rows, k]) - device tensors - of
    entry(*lead, k, exclude_known, *mid, idx_out, val_out, stream)."""
    idx = torch.empty(n_rows, k, dtype=torch.int32, device=device)
    val = torch.empty(n_rows, k, dtype=torch.float32, device=device)
    with ctx:
        _check(entry(*map(_arg, lead), int(k), int(bool(exclude_known)), *map(_arg, mid), _ptr(idx), _ptr(val),
                     _stream_of(device)))
    return idx, val


def _ranks_call(entry, device, ctx, n_truth, exclude_known, lead, mid=()):
    """int32 device tensor [n_truth] of entry(*lead, exclude_known, *mid, ranks_out, stream), lead ending in the truth batch;
    nothing is called where there is no truth entry."""
    ranks = torch.empty(int(n_truth), dtype=torch.int32, device=device)
    if n_truth:
        with ctx:
            _check(entry(*map(_arg, lead), int(bool(exclude_known)), *map(_arg, mid), _ptr(ranks), _stream_of(device)))
    return ranks


def _cooc_scores(entry, dtype, cooc, csr, row_start, n_rows, rows, out):
    out = _scratch(cooc.device, n_rows, int(cooc.shape[1]), out, dtype, "scratch", False)
    c, b = cooc.struct(), _csr_batch(csr, row_start, n_rows, rows)
    with torch.cuda.device(cooc.device):
        _check(getattr(load_library(), entry)(C.byref(c), int(cooc.shape[1]), C.byref(b), _ptr(out), out.stride(0),
                                              _stream_of(cooc.device)))
    return out[:n_rows, :cooc.shape[1]]


def _cooc_topk(entry, dtype, cooc, csr, row_start, n_rows, k, rows, exclude_known, scratch):
    n_items = int(cooc.shape[1])
    scratch = _scratch(cooc.device, n_rows, n_items, scratch, dtype, "scratch", False)
    lead = (cooc.struct(), n_items, _csr_batch(csr, row_start, n_rows, rows))
    return _list_call(getattr(load_library(), entry), cooc.device, torch.cuda.device(cooc.device), n_rows, k, exclude_known,
                      lead, (scratch, scratch.stride(0)))


def _cooc_ranks(entry, dtype, cooc, csr, row_start, n_rows, truth_csr, n_truth, rows, exclude_known, scratch):
    n_items = int(cooc.shape[1])
    scratch = _scratch(cooc.device, n_rows, n_items, scratch, dtype, "scratch", False)
    lead = (cooc.struct(), n_items, _csr_batch(csr, row_start, n_rows, rows), _csr_batch(truth_csr, row_start, n_rows, rows))
    return _ranks_call(getattr(load_library(), entry), cooc.device, torch.cuda.device(cooc.device), n_truth, exclude_known,
                       lead, (scratch, scratch.stride(0)))


def cooc_scores(cooc, csr, row_start, n_rows, rows=None, out=None):
    """float32 device tensor [n_rows, items]: X[rows] @ C for rows [row_start, row_start + n_rows) of the DeviceCSR `csr`
    (or the rows named by the int32 device tensor `rows`) - exact whole numbers while they stay below 2^24."""
    return _cooc_scores("aae_cooc_scores", torch.float32, cooc, csr, row_start, n_rows, rows, out)


def cooc_topk(cooc, csr, row_start, n_rows, k, rows=None, exclude_known=True, scratch=None):
    """(ids int32 [n_rows, k], scaled scores float32 [n_rows, k]) - device tensors: predict -> remove_non_missing -> argtopk
    of the co-occurrence scores, the better score first and the smaller id at equal scores (aae_cooc_topk)."""
    return _cooc_topk("aae_cooc_topk", torch.float32, cooc, csr, row_start, n_rows, k, rows, exclude_known, scratch)


def cooc_ranks(cooc, csr, row_start, n_rows, truth_csr, n_truth, rows=None, exclude_known=True, scratch=None):
    """int32 device tensor [n_truth]: the 1-based rank of every stored entry of the truth rows (the rows of `truth_csr` with
    the addressing of the input rows; n_truth = their stored entries), CSR order, in cooc_topk's ordering (aae_cooc_ranks)."""
    return _cooc_ranks("aae_cooc_ranks", torch.float32, cooc, csr, row_start, n_rows, truth_csr, n_truth, rows, exclude_known, scratch)


# The same three calls over an int32 score matrix / scratch (aae_cooc_*_i32): the scores are ranked as the integers they are, so
# ids and ranks are exact while every row keeps sum_i |x_i| * max_j |C_ij| < 2^31 - the caller's guarantee (aaerec.cooc.device_route),
# which the calls do not check.
def cooc_scores_i32(cooc, csr, row_start, n_rows, rows=None, out=None):
    """cooc_scores with an int32 result [n_rows, items]: the sums as they are."""
    return _cooc_scores("aae_cooc_scores_i32", torch.int32, cooc, csr, row_start, n_rows, rows, out)


def cooc_topk_i32(cooc, csr, row_start, n_rows, k, rows=None, exclude_known=True, scratch=None):
    """cooc_topk ranked on the int32 scores (`scratch`: int32); the scaled scores are (float(v) - float(min)) / span in fp32."""
    return _cooc_topk("aae_cooc_topk_i32", torch.int32, cooc, csr, row_start, n_rows, k, rows, exclude_known, scratch)


def cooc_ranks_i32(cooc, csr, row_start, n_rows, truth_csr, n_truth, rows=None, exclude_known=True, scratch=None):
    """cooc_ranks counted on the int32 scores (`scratch`: int32)."""
    return _cooc_ranks("aae_cooc_ranks_i32", torch.int32, cooc, csr, row_start, n_rows, truth_csr, n_truth, rows, exclude_known, scratch)


# ---- the exact int32 sparse product (aae_spgemm_i32_*; csrc/spgemm.h) -----------------------------------------------
def _spgemm_operands(A, B):
    if A.shape[1] != B.shape[0]:
        raise ValueError("aaerec: spgemm_i32 of [{} x {}] and [{} x {}]".format(*A.shape, *B.shape))
    if A.device != B.device:
        raise ValueError("aaerec: the operands of spgemm_i32 live on different devices")
    return A.struct(), B.struct(), C.c_void_p(torch.cuda.current_stream(A.device).cuda_stream)


def spgemm_bound(A, B):
    """int64 device tensor [rows of A]: u_i = the products of row i of A . B (aae_spgemm_i32_bound) - rows with
    u_i <= SPGEMM_HASH_PRODUCTS take the hash kernel, longer ones the tile kernel."""
    a, b, stream = _spgemm_operands(A, B)
    u = torch.empty(max(1, A.shape[0]), dtype=torch.int64, device=A.device)
    with torch.cuda.device(A.device):
        _check(load_library().aae_spgemm_i32_bound(C.byref(a), C.byref(b), int(B.shape[0]), _ptr(u), stream))
    return u[:A.shape[0]]


def spgemm_i32(A, B):
    """A . B as a DeviceCooc, exact in int32, the columns ascending in every row.  A, B: DeviceCooc-like (int32 CSR in HBM,
    canonical, strictly positive values whose products' sums stay below 2^31 - the caller's guarantee, not checked).  Two
    passes: Count, a cumsum, Fill; the one host read is nnz of the result, unknown until Count has run."""
    a, b, stream = _spgemm_operands(A, B)
    m, n, dev = int(A.shape[0]), int(B.shape[1]), A.device
    lib = load_library()
    u = torch.empty(max(1, m), dtype=torch.int64, device=dev)
    row_nnz = torch.zeros(max(1, m), dtype=torch.int64, device=dev)
    indptr = torch.zeros(m + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _check(lib.aae_spgemm_i32_bound(C.byref(a), C.byref(b), int(B.shape[0]), _ptr(u), stream))
        _check(lib.aae_spgemm_i32_count(C.byref(a), C.byref(b), n, _ptr(u), _ptr(row_nnz), stream))
        if m:
            torch.cumsum(row_nnz[:m], 0, out=indptr[1:])
        nnz = int(indptr[-1])
        indices = torch.empty(max(1, nnz), dtype=torch.int32, device=dev)
        values = torch.empty(max(1, nnz), dtype=torch.int32, device=dev)
        _check(lib.aae_spgemm_i32_fill(C.byref(a), C.byref(b), n, _ptr(u), _ptr(indptr), _ptr(indices), _ptr(values), stream))
    return DeviceCooc.from_device(indptr, indices, values, (m, n), dev)


# ---- the device CSR transpose (aae_csr_transpose_*; csrc/sptrans.h) -------------------------------------------------
def _transpose_arrays(indptr, indices, values, shape, device):
    """(indptr int64 [cols + 1], indices int32, values of values.dtype) of the transpose of the canonical CSR arrays on
    `device`: Count, a cumsum, Fill.  The values are moved as bits.  One host read: nnz of the result."""
    m, n, dev = int(shape[0]), int(shape[1]), torch.device(device)
    lib = load_library()
    col_nnz = torch.zeros(max(1, n), dtype=torch.int64, device=dev)
    t_indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _check(lib.aae_csr_transpose_count(_ptr(indptr), _ptr(indices), m, n, _ptr(col_nnz), stream))
        if n:
            torch.cumsum(col_nnz[:n], 0, out=t_indptr[1:])
        nnz = int(t_indptr[-1])
        t_indices = torch.empty(max(1, nnz), dtype=torch.int32, device=dev)
        t_values = torch.zeros(max(1, nnz), dtype=values.dtype, device=dev)
        scratch = torch.empty(nnz, dtype=torch.int64, device=dev) if nnz > SPTRANS_LDS else None
        _check(lib.aae_csr_transpose_fill(_ptr(indptr), _ptr(indices), _ptr(values), m, n, _ptr(t_indptr), _ptr(t_indices),
                                          _ptr(t_values), _ptr(col_nnz), _ptr(scratch), nnz if scratch is not None else 0, nnz, stream))
    return t_indptr, t_indices, t_values, nnz


def csr_transpose(csr):
    """The transpose of a canonical DeviceCSR (columns ascending and duplicate-free within a row) as a DeviceCSR: bit for bit
    scipy's A.T.tocsr() after sort_indices() (aae_csr_transpose_count / _fill).  A column id outside [0, cols) is skipped."""
    if csr.values.dtype != torch.float32 or csr.indices.dtype != torch.int32 or csr.indptr.dtype != torch.int64:
        raise TypeError("aaerec: csr_transpose takes a DeviceCSR (int64 indptr, int32 indices, float32 values)")
    dev = csr.indptr.device
    indptr, indices, values, nnz = _transpose_arrays(csr.indptr, csr.indices, csr.values, csr.shape, dev)
    out = DeviceCSR.__new__(DeviceCSR)
    out.generation = next(_GENERATION)
    out.shape = (int(csr.shape[1]), int(csr.shape[0]))
    out.nnz = nnz
    out.nnz_per_row_max = int(indptr.diff().max()) if out.shape[0] else 0
    out.indptr, out.indices, out.values = indptr, indices, values
    return out


def cooc_transpose(cooc):
    """The transpose of a DeviceCooc as a DeviceCooc: csr_transpose for the int32 operands of spgemm_i32."""
    indptr, indices, values, _ = _transpose_arrays(cooc.indptr, cooc.indices, cooc.values, cooc.shape, cooc.device)
    return DeviceCooc.from_device(indptr, indices, values, (cooc.shape[1], cooc.shape[0]), cooc.device)


# ---- mutual information of an unstored contingency table (aae_mi_i32_*; csrc/mutinfo.h) -----------------------------
def mutual_info_i32(A, B):
    """(mi, T, row_s1, row_pi) of the contingency table C = A . B, which is never stored: mi a float (base e, scikit-learn's
    mutual_info_score(contingency=C)), T = sum C an int, row_s1 [rows of A] float64 and row_pi [rows of A] int64 device tensors
    (S1_i = sum_j c_ij (ln c_ij - ln pj_j), pi_i = sum_j c_ij).  A = X^T, B = Y: DeviceCooc (int32 CSR in HBM, canonical,
    strictly positive values, every c_ij below 2^31 and T below 2^53 - the caller's guarantee, aaerec.utils.device_mi_ok).
    The same bits every run.  One host read: the 16 bytes of (mi, T).  Operands without an entry launch nothing."""
    a, b, stream = _spgemm_operands(A, B)
    m, p, n, dev = int(A.shape[0]), int(B.shape[0]), int(B.shape[1]), A.device
    row_s1 = torch.zeros(m, dtype=torch.float64, device=dev)
    row_pi = torch.zeros(m, dtype=torch.int64, device=dev)
    if m == 0 or p == 0 or n == 0 or A.nnz == 0 or B.nnz == 0:
        return 0.0, 0, row_s1, row_pi
    lib = load_library()
    u = torch.empty(m, dtype=torch.int64, device=dev)
    ints = torch.empty(p + n, dtype=torch.int64, device=dev)                    # a [p], pj [n]
    lnpj = torch.empty(n, dtype=torch.float64, device=dev)
    out = torch.empty(2, dtype=torch.int64, device=dev)                         # the bits of (double mi, int64 T)
    with torch.cuda.device(dev):
        _check(lib.aae_spgemm_i32_bound(C.byref(a), C.byref(b), p, _ptr(u), stream))
        _check(lib.aae_mi_i32_marginals(C.byref(a), C.byref(b), p, n, _ptr(ints), _ptr(ints[p:]), _ptr(lnpj), stream))
        _check(lib.aae_mi_i32_rows(C.byref(a), C.byref(b), n, _ptr(u), _ptr(lnpj), _ptr(row_s1), _ptr(row_pi), stream))
        _check(lib.aae_mi_i32_finish(m, _ptr(row_s1), _ptr(row_pi), _ptr(out), stream))
        host = out.cpu().numpy()
    return float(host[:1].view(np.float64)[0]), int(host[1]), row_s1, row_pi


# ---- the most-popular baseline (aae_pop_*; csrc/popular.h) ----------------------------------------------------------
def pop_counts(X):
    """int32 device tensor [items]: the column sums of the DeviceCooc `X` (a training matrix as int32 CSR in HBM), integer adds
    only (aae_pop_counts).  The caller keeps every column's absolute sum below 2^31 (aaerec.popular.device_count_ok)."""
    n_items = int(X.shape[1])
    counts = torch.empty(n_items, dtype=torch.int32, device=X.device)
    x = X.struct()
    with torch.cuda.device(X.device):
        _check(load_library().aae_pop_counts(C.byref(x), n_items, _ptr(counts), _stream_of(X.device)))
    return counts


class DevicePopular:
    """The item counts resident in HBM with the one order every row is ranked from: int32 `counts` [items], `order` - the
    ids by (count descending, id ascending) - and `pos`, its inverse.  counts: an int32 device tensor (pop_counts) or a host
    array of whole numbers below 2^31, uploaded once.  The order is a stable descending torch.sort on the device and `pos` a
    scatter: plumbing, done once per train()."""

    def __init__(self, counts, device):
        self.device = torch.device(device)
        if not torch.is_tensor(counts):
            counts = upload(np.ascontiguousarray(np.rint(np.asarray(counts).ravel()).astype(np.int32)), self.device)
        if not counts.is_cuda or counts.dtype != torch.int32 or counts.dim() != 1 or not counts.is_contiguous() or counts.numel() < 1:
            raise TypeError("aaerec: counts must be a contiguous int32 GPU vector of at least one item")
        self.counts = counts
        self.n_items = int(counts.numel())
        order = torch.sort(counts, descending=True, stable=True).indices
        self.order = order.to(torch.int32)
        self.pos = torch.empty(self.n_items, dtype=torch.int32, device=counts.device)
        self.pos[order] = torch.arange(self.n_items, dtype=torch.int32, device=counts.device)

    def struct(self):
        p = AaePopular()
        p.counts_dev, p.order_dev, p.pos_dev = self.counts.data_ptr(), self.order.data_ptr(), self.pos.data_ptr()
        p.n_items = self.n_items
        return p


def pop_topk(pop, csr, row_start, n_rows, k, rows=None, exclude_known=True):
    """(ids int32 [n_rows, k], scaled scores float32 [n_rows, k]) - device tensors: the first k items of the DevicePopular's
    order that a row of the DeviceCSR `csr` does not hold, for rows [row_start, row_start + n_rows) (or the rows named by the
    int32 device tensor `rows`); every k in [1, items] (aae_pop_topk)."""
    lead = (pop.struct(), _csr_batch(csr, row_start, n_rows, rows))
    return _list_call(load_library().aae_pop_topk, pop.device, torch.cuda.device(pop.device), n_rows, k, exclude_known, lead)


def pop_ranks(pop, csr, row_start, n_rows, truth_csr, n_truth, rows=None, exclude_known=True):
    """int32 device tensor [n_truth]: the 1-based rank of every stored entry of the truth rows (the rows of `truth_csr` with
    the addressing of the input rows; n_truth = their stored entries), CSR order, in pop_topk's ordering (aae_pop_ranks)."""
    lead = (pop.struct(), _csr_batch(csr, row_start, n_rows, rows), _csr_batch(truth_csr, row_start, n_rows, rows))
    return _ranks_call(load_library().aae_pop_ranks, pop.device, torch.cuda.device(pop.device), n_truth, exclude_known, lead)


# ---- the random baseline (aae_rand_*; csrc/randrank.h) --------------------------------------------------------------------
RAND_BITS = 24            # bits of a draw: the most a float32 score holds exactly
RAND_TRUTH_MAX = 4096     # most held-out items of a row aae_rand_ranks sorts in LDS (csrc/randrank.h kRandTruthMax)


def _rand_lead(seed, draw, row0, bits, n_items):
    return (C.c_uint64(int(seed) & (2 ** 64 - 1)), int(draw), int(row0), int(bits), int(n_items))


def rand_scores(seed, draw, row0, n_rows, n_items, device, bits=RAND_BITS, out=None):
    """float32 device matrix [n_rows, >= n_items]: the scores of rows [row0, row0 + n_rows) of draw number `draw` under `seed`,
    s * 2^-bits with s the top `bits` bits of the generator's word for (row, item) (aae_rand_scores).  out: the caller's matrix."""
    device = torch.device(device)
    out = _scratch(device, n_rows, int(n_items), out, torch.float32, "out", False)
    with torch.cuda.device(device):
        _check(load_library().aae_rand_scores(*_rand_lead(seed, draw, row0, bits, n_items), int(n_rows), _ptr(out), int(out.stride(0)),
                                              _stream_of(device)))
    return out


def rand_topk(seed, draw, row0, n_items, csr, row_start, n_rows, k, rows=None, exclude_known=True, bits=RAND_BITS):
    """(ids int32 [n_rows, k], scaled scores float32 [n_rows, k]) - device tensors: per row the k items with the largest draws that
    the row of the DeviceCSR `csr` does not hold, for rows [row_start, row_start + n_rows) (or the rows named by the int32 device
    tensor `rows`), which are rows row0 .. of the test set for the generator; k in [1, min(RANK_K_MAX, items)] (aae_rand_topk)."""
    device = csr.indptr.device
    lead = _rand_lead(seed, draw, row0, bits, n_items) + (_csr_batch(csr, row_start, n_rows, rows),)
    return _list_call(load_library().aae_rand_topk, device, torch.cuda.device(device), n_rows, k, exclude_known, lead)


def rand_ranks(seed, draw, row0, n_items, csr, row_start, n_rows, truth_csr, n_truth, rows=None, exclude_known=True, bits=RAND_BITS):
    """int32 device tensor [n_truth]: the 1-based rank of every stored entry of the truth rows (the rows of `truth_csr` with the
    addressing of the input rows, at most RAND_TRUTH_MAX entries each; n_truth = their stored entries), CSR order, in rand_topk's
    ordering (aae_rand_ranks)."""
    device = csr.indptr.device
    lead = _rand_lead(seed, draw, row0, bits, n_items) + (_csr_batch(csr, row_start, n_rows, rows),
                                                          _csr_batch(truth_csr, row_start, n_rows, rows))
    return _ranks_call(load_library().aae_rand_ranks, device, torch.cuda.device(device), n_truth, exclude_known, lead)


# ---- ranking metrics from held-out ranks (aae_metric_*, aae_ranks_from_lists; csrc/rank_metrics.h) ------------------------------
def discount_table(K):
    """float64 [K]: d[i] = 1 / log2(1 + i) at index i - 1, with the reference's own expression (eval/mpd/mpd_metrics.py:80)."""
    return 1.0 / np.log2(1 + np.arange(1, int(K) + 1))


class DeviceDiscounts:
    """The ndcg discount table resident in HBM, one per device: built on the host by discount_table and uploaded when a call needs
    more entries than the table kept so far holds, which it then replaces - d[i] sits at index i - 1 whatever the length, so the
    longest table asked for serves every smaller K with the same doubles."""
    _tables = {}

    @classmethod
    def get(cls, K, device):
        K, dev = int(K), torch.device(device)
        if not 1 <= K <= METRIC_NDCG_K_MAX:
            raise ValueError("a discount table holds 1 to {} entries, not {}".format(METRIC_NDCG_K_MAX, K))
        key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
        if key not in cls._tables or cls._tables[key].numel() < K:
            cls._tables[key] = upload(discount_table(K), dev)
        return cls._tables[key]


def rank_metrics(indptr, ranks, specs, per_row=False):
    """The metrics `specs` - [(kind, k)], kind a METRIC_KINDS value, k = 0 unbounded - of the rows of held-out ranks on the
    device: indptr int64 [n + 1], ranks int32 in CSR order (as the *_ranks calls and ranks_from_lists write them), both device
    tensors.  float64 host array [len(specs), 2] of (mean, population std) - the only bytes that leave the device - or, with
    per_row, [len(specs), n].  The caller keeps every row within METRIC_ROW_MAX entries, every rank >= 1 and every ndcg k
    within METRIC_NDCG_K_MAX (aaerec.evaluation does): a row beyond that comes back NaN."""
    dev = indptr.device
    if not (indptr.is_cuda and ranks.is_cuda and indptr.dtype == torch.int64 and ranks.dtype == torch.int32
            and indptr.is_contiguous() and ranks.is_contiguous() and indptr.numel() >= 1):
        raise TypeError("aaerec: indptr / ranks must be contiguous int64 / int32 GPU vectors")
    specs = [(int(kind), int(k)) for kind, k in specs]
    n, lib = int(indptr.numel()) - 1, load_library()
    if ranks.numel() == 0:
        ranks = torch.zeros(1, dtype=torch.int32, device=dev)        # (a valid pointer: nothing reads it)
    kd = max([k for kind, k in specs if kind == METRIC_KINDS["ndcg"]], default=0)
    disc = DeviceDiscounts.get(kd, dev) if kd else None
    rows = AaeRankRows()
    rows.indptr_dev, rows.ranks_dev, rows.n_rows = indptr.data_ptr(), ranks.data_ptr(), n
    vals = torch.empty(len(specs), max(n, 1), dtype=torch.float64, device=dev)
    out = torch.empty(len(specs), 2, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        stream = _stream_of(dev)
        for q0 in range(0, len(specs), METRIC_MAX):
            part = specs[q0:q0 + METRIC_MAX]
            arr = (AaeMetricSpec * len(part))(*[AaeMetricSpec(kind, k) for kind, k in part])
            _check(lib.aae_metric_rows(C.byref(rows), arr, len(part), _ptr(disc), 0 if disc is None else int(disc.numel()), _ptr(vals[q0:]),
                                       vals.stride(0), stream))
            if not per_row:
                _check(lib.aae_metric_finish(_ptr(vals[q0:]), vals.stride(0), n, len(part), _ptr(out[q0:]), stream))
    return vals[:, :n].cpu().numpy() if per_row else out.cpu().numpy()


def ranks_from_lists(ids, truth_csr, row_start, n_rows, n_truth, k=None, rows=None):
    """int32 device tensor [n_truth]: for every stored entry of the truth rows (DeviceCSR `truth_csr`, canonical; rows
    [row_start, row_start + n_rows) or those named by `rows`; n_truth their stored entries), CSR order, its position + 1 among
    the first k ids of its row of `ids` (int32 device tensor [n_rows, >= k], best first, -1 padding) or RANK_ABSENT."""
    if not ids.is_cuda or ids.dtype != torch.int32 or ids.dim() != 2 or ids.stride(1) != 1 or ids.shape[0] < n_rows:
        raise TypeError("aaerec: ids must be an int32 GPU matrix [n_rows, k] with unit column stride")
    k = int(ids.shape[1] if k is None else k)
    if not 1 <= k <= ids.shape[1]:
        raise ValueError("k must be in [1, {}]".format(ids.shape[1]))
    out = torch.empty(int(n_truth), dtype=torch.int32, device=ids.device)
    if n_truth and n_rows:
        b = _csr_batch(truth_csr, row_start, n_rows, rows)
        with torch.cuda.device(ids.device):
            _check(load_library().aae_ranks_from_lists(_ptr(ids), int(ids.stride(0)), k, C.byref(b), _ptr(out), _stream_of(ids.device)))
    return out


def spmm_f32(csr, dense, width=None, out=None):
    """float32 device tensor [rows, width]: csr @ dense[:, :width] for the DeviceCSR `csr` [rows, cols] and the float32 GPU
    matrix `dense` [cols, >= width] (unit column stride, a 16-byte aligned base, a row stride that is a multiple of 4 floats and
    at least width rounded up to 4 - the padding is read) (aae_spmm_f32: the projection kernel of csrc/lowrank.h, one k-ordered
    fmaf chain per element in CSR order).  out: a matrix of the same kind of at least [rows, width], or a new one."""
    width = int(dense.shape[1] if width is None else width)
    n_rows, n_cols = int(csr.shape[0]), int(csr.shape[1])
    if not dense.is_cuda or dense.dtype != torch.float32 or dense.dim() != 2 or dense.stride(1) != 1 or dense.shape[0] < n_cols \
            or dense.shape[1] < width:
        raise TypeError("aaerec: dense must be a float32 GPU matrix of [cols of csr, >= width] with unit column stride")
    dev = dense.device
    if out is None:
        out = torch.empty(n_rows, (max(width, 1) + 3) & ~3, dtype=torch.float32, device=dev)
    elif not out.is_cuda or out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] < n_rows:
        raise TypeError("aaerec: out must be a float32 GPU matrix of at least [rows of csr, width] with unit column stride")
    b = _csr_batch(csr, 0, n_rows)
    with torch.cuda.device(dev):
        _check(load_library().aae_spmm_f32(C.byref(b), _ptr(dense), dense.stride(0), n_cols, width, _ptr(out), out.stride(0),
                                           C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return out[:n_rows, :width]


# ---- the truncated-SVD baseline (aae_lowrank_*; csrc/lowrank.h) -----------------------------------------------------
class DeviceLowRank:
    """TruncatedSVD.components_ [dims, features] resident in HBM as the kernels read it: ONE float32 table Vt
    [features, ld], row f = column f of the components, ld = dims rounded up to 4 floats, the padding zero."""

    def __init__(self, components, device):
        V = np.asarray(components)
        if V.ndim != 2 or not 1 <= V.shape[0] <= LOWRANK_DIMS_MAX or V.shape[1] < 1:
            raise ValueError("aaerec: components must be [dims, features] with dims in [1, %d]" % LOWRANK_DIMS_MAX)
        dims, features = V.shape
        vt = np.zeros((features, (dims + 3) & ~3), dtype=np.float32)
        vt[:, :dims] = V.T
        self.shape = (features, dims)
        self.device = torch.device(device)
        self.table = upload(vt, device)

    def struct(self):
        s = AaeLowRank()
        s.vt_dev, s.ld = self.table.data_ptr(), self.table.stride(0)
        s.n_features, s.dims = int(self.shape[0]), int(self.shape[1])
        return s


def _lowrank_buffers(lr, n_rows, n_items, scratch, hidden, what="scratch"):
    return _scratch(lr.device, n_rows, int(n_items), scratch, torch.float32, what, True), \
        _scratch(lr.device, n_rows, lr.shape[1], hidden, torch.float32, "hidden", True)


def lowrank_scores(lr, n_items, csr, row_start, n_rows, rows=None, out=None, hidden=None):
    """float32 device tensor [n_rows, n_items]: (X[rows] Vt) Vt[:n_items]^T for rows [row_start, row_start + n_rows) of the
    DeviceCSR `csr` of feature rows (or the rows named by the int32 device tensor `rows`) (aae_lowrank_scores)."""
    out, hidden = _lowrank_buffers(lr, n_rows, n_items, out, hidden, "out")
    v, b = lr.struct(), _csr_batch(csr, row_start, n_rows, rows)
    with torch.cuda.device(lr.device):
        _check(load_library().aae_lowrank_scores(C.byref(v), int(n_items), C.byref(b), _ptr(hidden), hidden.stride(0), _ptr(out),
                                                 out.stride(0), _stream_of(lr.device)))
    return out[:n_rows, :n_items]


def lowrank_topk(lr, n_items, csr, items_csr, row_start, n_rows, k, rows=None, exclude_known=True, scratch=None, hidden=None):
    """(ids int32 [n_rows, k], scaled scores float32 [n_rows, k]) - device tensors: predict -> remove_non_missing -> argtopk of
    the truncated-SVD scores of the feature rows `csr`; `items_csr` names the known items of the same rows (ids below
    n_items).  The better score first, the smaller id at equal scores (aae_lowrank_topk)."""
    scratch, hidden = _lowrank_buffers(lr, n_rows, n_items, scratch, hidden)
    lead = (lr.struct(), int(n_items), _csr_batch(csr, row_start, n_rows, rows), _csr_batch(items_csr, row_start, n_rows, rows))
    return _list_call(load_library().aae_lowrank_topk, lr.device, torch.cuda.device(lr.device), n_rows, k, exclude_known,
                      lead, (hidden, hidden.stride(0), scratch, scratch.stride(0)))


def lowrank_ranks(lr, n_items, csr, items_csr, row_start, n_rows, truth_csr, n_truth, rows=None, exclude_known=True, scratch=None,
                  hidden=None):
    """int32 device tensor [n_truth]: the 1-based rank of every stored entry of the truth rows (the rows of `truth_csr` with
    the addressing of the input rows; n_truth = their stored entries), CSR order, in lowrank_topk's ordering
    (aae_lowrank_ranks)."""
    scratch, hidden = _lowrank_buffers(lr, n_rows, n_items, scratch, hidden)
    lead = (lr.struct(), int(n_items), _csr_batch(csr, row_start, n_rows, rows), _csr_batch(items_csr, row_start, n_rows, rows),
            _csr_batch(truth_csr, row_start, n_rows, rows))
    return _ranks_call(load_library().aae_lowrank_ranks, lr.device, torch.cuda.device(lr.device), n_truth, exclude_known,
                       lead, (hidden, hidden.stride(0), scratch, scratch.stride(0)))


# ---- IRGAN (aae_irgan_*; csrc/irgan.h) -------------------------------------------------------------------------------
IRGAN_KEYS = ("user_emb", "item_emb", "item_bias", "m_user_emb", "m_item_emb", "m_item_bias")


class DeviceIrganNet:
    """One net of IRGAN in HBM: user_emb [users, dim], item_emb [items, dim], item_bias [items] and their momentum buffers, fp32,
    contiguous.  arrays: the six by IRGAN_KEYS (a missing momentum buffer is zeros)."""

    def __init__(self, arrays, device):
        self.device = torch.device(device)
        u, v, b = (np.asarray(arrays[k], dtype=np.float32) for k in IRGAN_KEYS[:3])
        if u.ndim != 2 or v.ndim != 2 or b.ndim != 1 or u.shape[1] != v.shape[1] or v.shape[0] != b.shape[0]:
            raise ValueError("aaerec: user_emb [users, dim], item_emb [items, dim] and item_bias [items] do not fit together")
        self.users, self.dim, self.items = int(u.shape[0]), int(u.shape[1]), int(v.shape[0])
        self.t = {}
        for k, p in zip(IRGAN_KEYS, (u, v, b, u, v, b)):
            a = np.asarray(arrays[k], dtype=np.float32) if arrays.get(k) is not None else np.zeros_like(p)
            if a.shape != p.shape:
                raise ValueError("aaerec: {} has shape {}, not {}".format(k, a.shape, p.shape))
            self.t[k] = upload(np.ascontiguousarray(a), self.device).contiguous()

    def struct(self):
        s = AaeIrganNet()
        for k in IRGAN_KEYS:
            setattr(s, k + "_dev", self.t[k].data_ptr())
        s.users, s.items, s.dim = self.users, self.items, self.dim
        return s

    def arrays(self):
        return {k: self.t[k].cpu().numpy() for k in IRGAN_KEYS}


def irgan_scratch(net, slots=1):
    """The uint8 scratch of the training calls of `net`: aae_irgan_scratch_bytes, with room for `slots` users' softmax tables
    (aae_irgan_sample_neg works on that many users per launch)."""
    n = C.c_size_t()
    s = net.struct()
    _check(load_library().aae_irgan_scratch_bytes(C.byref(s), C.byref(n)))
    tiles = (net.items + IRGAN_TILE - 1) // IRGAN_TILE
    extra = (max(1, int(slots)) - 1) * tiles * (24 + 4 * IRGAN_TILE)
    return torch.empty(n.value + extra + 256, dtype=torch.uint8, device=net.device)


def _irgan_scratch_arg(scratch):
    off = (-scratch.data_ptr()) % 256
    return C.c_void_p(scratch.data_ptr() + off), C.c_size_t(scratch.numel() - off)


def irgan_scores(net, users, pos=None, out=None):
    """float32 device tensor [len(users), items]: the logits of the int32 device tensor `users`, 0 at the training positives
    `pos` = (indptr int64 [users + 1], ascending item ids int32) device tensors, or None (aae_irgan_scores)."""
    n = int(users.numel())
    out = _scratch(net.device, n, net.items, out, torch.float32, "out", True)
    s = net.struct()
    with torch.cuda.device(net.device):
        _check(load_library().aae_irgan_scores(C.byref(s), _ptr(users), n, _ptr(pos[0]) if pos else None, _ptr(pos[1]) if pos else None,
                                               _ptr(out), out.stride(0), _stream_of(net.device)))
    return out[:n, :net.items]


def irgan_topk(net, users, pos, known_csr, row_start, n_rows, k, exclude_known=True, scratch=None):
    """(ids int32 [n_rows, k], scaled scores float32 [n_rows, k]) - device tensors - of rows [row_start, row_start + n_rows) of
    the DeviceCSR `known_csr` (the test rows' known items), row r scored as user users[r] (aae_irgan_topk)."""
    scratch = _scratch(net.device, n_rows, net.items, scratch, torch.float32, "scratch", True)
    lead = (net.struct(), users, pos[0] if pos else None, pos[1] if pos else None, _csr_batch(known_csr, row_start, n_rows))
    return _list_call(load_library().aae_irgan_topk, net.device, torch.cuda.device(net.device), n_rows, k, exclude_known, lead,
                      (scratch, scratch.stride(0)))


def irgan_ranks(net, users, pos, known_csr, row_start, n_rows, truth_csr, n_truth, exclude_known=True, scratch=None):
    """int32 device tensor [n_truth]: the 1-based ranks of the stored entries of the truth rows, CSR order (aae_irgan_ranks)."""
    scratch = _scratch(net.device, n_rows, net.items, scratch, torch.float32, "scratch", True)
    lead = (net.struct(), users, pos[0] if pos else None, pos[1] if pos else None, _csr_batch(known_csr, row_start, n_rows),
            _csr_batch(truth_csr, row_start, n_rows))
    return _ranks_call(load_library().aae_irgan_ranks, net.device, torch.cuda.device(net.device), n_truth, exclude_known, lead,
                       (scratch, scratch.stride(0)))


def irgan_d_steps(net, lines, batch_size, n_steps, lr, momentum, lam, scratch, losses=False):
    """n_steps D steps over the int32 device tensor `lines` [n, 3] (aae_irgan_d_steps); the fp64 device tensor of the steps'
    losses when asked for."""
    out = torch.empty(n_steps, dtype=torch.float64, device=net.device) if losses else None
    s = net.struct()
    p, nb = _irgan_scratch_arg(scratch)
    with torch.cuda.device(net.device):
        _check(load_library().aae_irgan_d_steps(C.byref(s), _ptr(lines), int(lines.shape[0]), int(batch_size), int(n_steps), float(lr),
                                                float(momentum), float(lam), _ptr(out), p, nb, _stream_of(net.device)))
    return out


def irgan_sample_neg(net, users, line_off, max_pos, temperature, seed, draw, lines, scratch):
    """generate_for_d: column 2 of the int32 device tensor `lines` [n, 3] for the users of the int32 device tensor `users`,
    user q owning lines [line_off[q], line_off[q + 1]) (int64 device tensor) (aae_irgan_sample_neg)."""
    s = net.struct()
    p, nb = _irgan_scratch_arg(scratch)
    with torch.cuda.device(net.device):
        _check(load_library().aae_irgan_sample_neg(C.byref(s), _ptr(users), _ptr(line_off), int(users.numel()), int(max_pos),
                                                   float(temperature), C.c_uint64(int(seed) & (2 ** 64 - 1)), int(draw), _ptr(lines),
                                                   int(lines.shape[0]), p, nb, _stream_of(net.device)))


def irgan_g_steps(gen, dis, users, pos, max_pos, lr, momentum, scratch, samples=None, sample_off=None, seed=0, draw=0, losses=False,
                  samples_out=None):
    """One G step per entry of the int32 device tensor `users`; samples injected (int32 `samples`, int64 `sample_off`) or drawn
    by (seed, draw), and then written to the int32 `samples_out` at `sample_off` if that is given (aae_irgan_g_steps).  The fp64
    device tensor of the steps' losses when asked for."""
    n = int(users.numel())
    out = torch.empty(n, dtype=torch.float64, device=gen.device) if losses else None
    g, d = gen.struct(), dis.struct()
    p, nb = _irgan_scratch_arg(scratch)
    with torch.cuda.device(gen.device):
        _check(load_library().aae_irgan_g_steps(C.byref(g), C.byref(d), _ptr(users), n, _ptr(pos[0]), _ptr(pos[1]), int(max_pos),
                                                _ptr(samples), _ptr(sample_off), _ptr(samples_out), C.c_uint64(int(seed) & (2 ** 64 - 1)),
                                                int(draw),
                                                float(lr), float(momentum), _ptr(out), p, nb, _stream_of(gen.device)))
    return out


# state_dict key <-> (net, layer)
_NETS = {"enc": 0, "dec": 1, "disc": 2}
_PARAM_ID = {("enc", 1): T_ENC_W1T, ("enc", 2): T_ENC_W2, ("enc", 3): T_ENC_W3,
             ("dec", 1): T_DEC_V1, ("dec", 2): T_DEC_V2, ("dec", 3): T_DEC_V3,
             ("disc", 1): T_DISC_D1, ("disc", 2): T_DISC_D2, ("disc", 3): T_DISC_D3}
_OPTIM_ID = {"enc": O_ENC, "dec": O_DEC, "gen": O_GEN, "disc": O_DISC}


class HipAAE:
    """One model replica on one GPU: owns the arena and the C handle."""

    def __init__(self, n_items, n_hidden, n_code, cond_inc=0, max_batch=100, max_nnz=None,
                 activation="ReLU", prior="gauss", prior_scale=None, optimizer="adam",
                 normalize_inputs=True, dropout=(.2, .2), gen_lr=1e-3, reg_lr=1e-3,
                 rng_mode="device", seed=0, grad_mode="fused", device=None, unfused_decoder=False,
                 dp_world=1, w1_cap=None, ae_only=False, vae=False, dtype="f32", blocked_output=False, dense_noise=False,
                 vae_wide=False):
        lib = load_library()
        if not torch.cuda.is_available():
            raise AaeHipError("no HIP device: the AAE step has no CPU fallback")
        if activation not in ACTIVATIONS:
            raise ValueError(f"activation {activation!r} has no gfx950 kernel (supported: {sorted(ACTIVATIONS)})")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.lib = lib
        cfg = AaeConfig()
        cfg.abi_version = ABI_VERSION
        cfg.n_items, cfg.n_hidden, cfg.n_code, cfg.cond_inc = n_items, n_hidden, n_code, cond_inc
        cfg.max_batch = max_batch
        # capacity of the per-batch scratch lists; the default allows 4096 entries per row
        cfg.max_nnz = int(max_nnz if max_nnz is not None else min(2 ** 31 - 1, max_batch * min(n_items, 4096)))
        cfg.activation = ACTIVATIONS[activation]
        cfg.enc_final = FINALS[{"gauss": "linear", "categorical": "softmax", "bernoulli": "sigmoid"}[prior]]
        cfg.optimizer = OPTIMIZERS[optimizer]
        cfg.normalize_inputs = int(bool(normalize_inputs))
        cfg.rng_mode = RNG_DEVICE if rng_mode == "device" else RNG_INJECT
        cfg.prior = PRIORS[prior]
        cfg.grad_mode = GRAD_EXPORT if grad_mode == "export" else GRAD_FUSED
        cfg.dropout1, cfg.dropout2 = float(dropout[0]), float(dropout[1])
        cfg.gen_lr, cfg.reg_lr = float(gen_lr), float(reg_lr)
        cfg.has_prior_scale = int(prior_scale is not None)
        cfg.prior_scale = float(prior_scale) if prior_scale is not None else 1.0
        cfg.seed = int(seed) & (2 ** 64 - 1)
        cfg.unfused_decoder = 1 if unfused_decoder else 0
        cfg.dp_world = int(dp_world) if grad_mode == "export" else 0
        cfg.model_kind = MODEL_VAE if vae else MODEL_AE if ae_only else MODEL_AAE
        if dtype not in ("f32", "bf16"):
            raise ValueError("dtype must be 'f32' or 'bf16'")
        cfg.dtype = DTYPE_BF16 if dtype == "bf16" else DTYPE_F32
        # batches beyond one fused launch's 112 rows as row-blocked launches of the fused output layer (up to 1664 rows;
        # DESIGN.md 3.1) instead of the three streaming GEMMs: what fit() asks for at such batch sizes and the item
        # slices of the sharded schemes always.  Both dtypes since late r4 (bf16 on the rounded-operand form of the same
        # kernels: C3's shape at batch 512 1.01 -> 0.56 ms/step, C4 0.50 -> 0.40)
        cfg.blocked_output = 1 if (blocked_output and grad_mode != "export") else 0
        # DenoisingAutoEncoder(corrupt='gauss'): room for the dense noisy encoder input (set_input_noise before a step)
        cfg.dense_noise = 1 if dense_noise else 0
        # a VAE handle's wide bounds (n_hidden <= VAE_WIDE_HIDDEN_MAX, n_code <= VAE_WIDE_CODE_MAX): beyond a chain slot - or under the
        # NO_CHAIN option - its hidden half runs one launch per layer; at sizes that fit a slot it is the handle of vae_wide=False
        cfg.vae_wide = 1 if vae_wide else 0
        self.dtype = dtype
        self.ae_only, self.vae = bool(ae_only or vae), bool(vae)
        self.dp_world = int(dp_world)
        # rows of the packed first-layer gradient one rank may send per exchange
        self.w1_cap = int(w1_cap if w1_cap is not None else min(cfg.max_nnz, n_items, 65536))
        self._w1_hdr = (1 + self.w1_cap + 3) & ~3          # int32 words of the packet header (16-byte aligned)
        self._w1_packet = None
        self.cfg = cfg
        self.N, self.h, self.c, self.cond_inc = n_items, n_hidden, n_code, cond_inc
        self.max_batch = max_batch
        nbytes = C.c_size_t()
        _check(lib.aae_arena_bytes(C.byref(cfg), C.byref(nbytes)))
        with self._on_device():
            self.arena = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            assert self.arena.data_ptr() % 256 == 0
            h = C.c_void_p()
            _check(lib.aae_create(C.byref(cfg), C.c_void_p(self.arena.data_ptr()), nbytes.value, self._stream(),
                                  C.byref(h)))
        self.handle = h
        # aae_destroy waits for the handle's side stream (the deferred dec_optim launch of the last step reads and writes
        # the arena): it must run BEFORE the arena's memory can go back to the driver - also at interpreter exit, where
        # __del__ is not guaranteed to.  The finalizer owns a reference to the arena, so the order is fixed.
        self._finalizer = weakref.finalize(self, _destroy_handle, lib, h, self.arena, os.getpid())
        _check(lib.aae_set_lr(self.handle, float(gen_lr), float(reg_lr)))
        self._keep = []   # device buffers of the running step
        self._ga1_ld = None
        self._ext_first = False
        self._rank_rows = {}

    def close(self):
        """Destroy the handle now (waits for its side stream)."""
        self._finalizer()
        self.handle = None

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _on_device(self):
        """Context with this handle's device current.  One process per GPU is the rule: the device is almost always
        current already, and torch.cuda.device()'s enter / exit (two runtime calls and a Python context per library call,
        ~30 calls per data-parallel step) is skipped then."""
        if torch.cuda.current_device() == self._dev_index:
            return _NULL_CTX
        return torch.cuda.device(self.device)

    # ---- views into the arena ---------------------------------------------------------
    def tensor(self, tid, padded=False):
        """float32 view [rows, cols] (strided by ld) of a tensor of the model.  (The current stream first waits for the
        deferred optimiser launch of the last step, if one is pending: a view is about to read or write what it touches.)"""
        if tid >= T_ACT_Z:          # activations: only the deferred optimiser launch reads them (a prefetch does not)
            _check(self.lib.aae_join_output_layer(self.handle, self._stream()))
        else:
            self.join()
        info = AaeTensor()
        _check(self.lib.aae_tensor_info(self.handle, tid, C.byref(info)))
        flat = self.arena[info.byte_offset: info.byte_offset + info.rows * info.ld * 4].view(torch.float32)
        full = flat.view(info.rows, info.ld)
        return full if padded else full[:, :info.cols]

    def _span(self, tid_lo, tid_hi):
        """One flat float32 view from the start of tensor tid_lo to the end of tid_hi (they are
        adjacent in the arena; the 256-byte alignment gaps in between are never written)."""
        self.join()
        a, b = AaeTensor(), AaeTensor()
        _check(self.lib.aae_tensor_info(self.handle, tid_lo, C.byref(a)))
        _check(self.lib.aae_tensor_info(self.handle, tid_hi, C.byref(b)))
        end = b.byte_offset + b.rows * b.ld * 4
        return self.arena[a.byte_offset:end].view(torch.float32)

    def grad_buckets(self, which):
        """Flat gradient views to all-reduce for optimiser `which` (export mode).  The first
        encoder layer's row-sparse gradient is not among them: see w1_export / w1_import."""
        if which in (O_ENC, O_GEN):
            return []        # b1, W2, W3 ride in the w1_export packet and are applied by w1_import
        if which == O_DEC:
            return [self._span(T_GRAD + T_DEC_V1, T_GRAD + T_DEC_V2), self._span(T_GRAD + T_DEC_V3, T_GRAD + T_DEC_V3)]
        if which == "dec_small":
            return [self._span(T_GRAD + T_DEC_V1, T_GRAD + T_DEC_V2)]
        if which == "enc_small":        # (first layer external: its bias, W2, W3)
            return [self._span(T_GRAD + T_ENC_B1, T_GRAD + T_ENC_W3)]
        if which == "enc_dec_small":    # b1, W2, W3, V1, V2: one contiguous span of the arena
            return [self._span(T_GRAD + T_ENC_B1, T_GRAD + T_DEC_V2)]
        return [self._span(T_GRAD + T_DISC_D1, T_GRAD + T_DISC_D3)]

    def params_changed(self):
        """Parameters were written through arena views: derived copies are rebuilt before their next use."""
        _check(self.lib.aae_params_changed(self.handle))

    def join(self):
        """Make the current stream wait for the last step's deferred dec_optim launch (aae_join; no-op when none)."""
        _check(self.lib.aae_join(self.handle, self._stream()))

    def set_lr(self, gen_lr, reg_lr):
        """The learning rates from the next step on (aae_set_lr): gen_lr for enc_optim / dec_optim, reg_lr for gen_optim / disc_optim."""
        with self._on_device():
            _check(self.lib.aae_set_lr(self.handle, float(gen_lr), float(reg_lr)))

    def set_split(self, workgroups):
        """0: the fused output layer as one launch on the caller's stream; n > 0: split form, n workgroups for the
        deferred dec_optim launch (aae_set_split)."""
        self.sync()
        _check(self.lib.aae_set_split(self.handle, int(workgroups)))

    # ---- state_dict in the reference layout ------------------------------------------
    def sync(self):
        """Replay the deferred W1T updates so that arena views show eager-equivalent values."""
        with self._on_device():
            _check(self.lib.aae_sync(self.handle, self._stream()))

    def load_params(self, params):
        """params: {'enc.lin1.weight': ndarray [out,in], 'enc.lin1.bias': ...} (any subset of layers,
        weight and bias together)."""
        self.sync()
        for (net, layer), tid in _PARAM_ID.items():
            wk, bk = f"{net}.lin{layer}.weight", f"{net}.lin{layer}.bias"
            if wk not in params:
                continue
            w = torch.as_tensor(np.asarray(params[wk], dtype=np.float32), device=self.device)
            b = torch.as_tensor(np.asarray(params[bk], dtype=np.float32), device=self.device)
            self._put(tid, w, b)
        torch.cuda.synchronize(self.device)
        _check(self.lib.aae_params_changed(self.handle))     # (written through arena views, not aae_load_linear)

    def _put(self, tid, w, b, tid_b1=T_ENC_B1):
        if self._is_w1t(tid):
            self.tensor(tid).copy_(w.t())
            self.tensor(tid_b1)[0].copy_(b)
        else:
            t = self.tensor(tid)
            t[:, :-1].copy_(w)
            t[:, -1].copy_(b)

    @staticmethod
    def _is_w1t(tid):
        return tid in (T_ENC_W1T, T_ADAM_ENC, T_ADAM_ENC + 1, T_ADAM_GEN, T_ADAM_GEN + 1)

    def _get(self, tid, tid_b1):
        if self._is_w1t(tid):
            return self.tensor(tid).t().contiguous().cpu().numpy(), self.tensor(tid_b1)[0].cpu().numpy().copy()
        t = self.tensor(tid)
        return t[:, :-1].contiguous().cpu().numpy(), t[:, -1].contiguous().cpu().numpy()

    def state_dict(self):
        self.sync()
        out = {}
        for (net, layer), tid in _PARAM_ID.items():
            w, b = self._get(tid, T_ENC_B1)
            out[f"{net}.lin{layer}.weight"], out[f"{net}.lin{layer}.bias"] = w, b
        return out

    def adam_state(self, which):
        """{'lin1.weight': (m, v), ...} of optimiser `which` in 'enc','dec','gen','disc', + step."""
        base, net, lo = {"enc": (T_ADAM_ENC, "enc", 0), "gen": (T_ADAM_GEN, "enc", 0),
                         "dec": (T_ADAM_DEC, "dec", 0), "disc": (T_ADAM_DISC, "disc", 0)}[which]
        self.sync()
        out = {}
        if net == "enc":
            slots = {1: 0, 2: 2, 3: 3}
            b1m, b1v = base + 2, base + 3
        else:
            slots = {1: 0, 2: 1, 3: 2}
        for layer, slot in slots.items():
            tm, tv = base + 2 * slot, base + 2 * slot + 1
            if net == "enc" and layer == 1:
                mw, mb = self._get(tm, b1m)
                vw, vb = self._get(tv, b1v)
            else:
                mw, mb = self._get(tm, None)
                vw, vb = self._get(tv, None)
            out[f"lin{layer}.weight"] = (mw, vw)
            out[f"lin{layer}.bias"] = (mb, vb)
        step = C.c_int64()
        oid = {"enc": O_ENC, "dec": O_DEC, "gen": O_GEN, "disc": O_DISC}[which]
        _check(self.lib.aae_store_adam(self.handle, oid, 2, None, None, None, None, C.byref(step)))
        out["step"] = step.value
        return out

    def load_adam_state(self, which, state):
        """The inverse of adam_state (aae_load_adam): state = {'lin1.weight': (m, v), 'lin1.bias': (m, v), ..., 'step': n}
        for optimiser `which` in 'enc','dec','gen','disc'; layers that are absent stay as they are, and so does the step
        count without a 'step' entry.  enc_optim and gen_optim share one count (include/aaerec_hip.h: aae_load_adam)."""
        oid = _OPTIM_ID[which]
        for layer in (1, 2, 3):
            wk, bk = f"lin{layer}.weight", f"lin{layer}.bias"
            if wk not in state and bk not in state:
                continue
            (mw, vw), (mb, vb) = state.get(wk, (None, None)), state.get(bk, (None, None))
            self.load_adam(oid, layer, mw, vw, mb, vb)
        if state.get("step") is not None:
            self.load_adam(oid, 2, step=int(state["step"]))

    # ---- the checkpoint entry points of the C ABI as they are: host arrays in the reference's layout ----
    def linear_shape(self, net, layer):
        """(out, in) of net 0 enc / 1 dec / 2 disc, layer 1..3 - the shape of the [out, in] weight aae_store_linear writes."""
        info = AaeTensor()
        _check(self.lib.aae_tensor_info(self.handle, _PARAM_ID[(("enc", "dec", "disc")[net], layer)], C.byref(info)))
        return (int(info.cols), int(info.rows)) if (net, layer) == (0, 1) else (int(info.rows), int(info.cols) - 1)

    @staticmethod
    def _host_in(a, shape, what):
        if a is None:
            return None, None
        a = np.ascontiguousarray(a, dtype=np.float32)
        if a.shape != shape:
            raise ValueError(f"{what}: shape {a.shape}, expected {shape}")
        return a, a.ctypes.data_as(C.c_void_p)

    def store_linear(self, net, layer, weight=True, bias=True):
        """aae_store_linear: (weight [out, in] or None, bias [out] or None) as numpy arrays."""
        out, inn = self.linear_shape(net, layer)
        w = np.empty((out, inn), dtype=np.float32) if weight else None
        b = np.empty((out,), dtype=np.float32) if bias else None
        with self._on_device():
            _check(self.lib.aae_store_linear(self.handle, net, layer, None if w is None else w.ctypes.data_as(C.c_void_p),
                                             None if b is None else b.ctypes.data_as(C.c_void_p)))
        return w, b

    def load_linear(self, net, layer, weight=None, bias=None):
        """aae_load_linear: weight [out, in] and / or bias [out] (None = left as it is)."""
        out, inn = self.linear_shape(net, layer)
        w, wp = self._host_in(weight, (out, inn), "weight")
        b, bp = self._host_in(bias, (out,), "bias")
        with self._on_device():
            _check(self.lib.aae_load_linear(self.handle, net, layer, wp, bp))

    def store_adam(self, which, layer, weight=True, bias=True, step=True):
        """aae_store_adam of optimiser id `which` (O_ENC ..): (m_w, v_w, m_b, v_b, step), None for what was not asked for."""
        out, inn = self.linear_shape({O_ENC: 0, O_GEN: 0, O_DEC: 1, O_DISC: 2}[which], layer)
        mw, vw = (np.empty((out, inn), dtype=np.float32) for _ in range(2)) if weight else (None, None)
        mb, vb = (np.empty((out,), dtype=np.float32) for _ in range(2)) if bias else (None, None)
        st = C.c_int64(-1)
        p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)           # noqa: E731
        with self._on_device():
            _check(self.lib.aae_store_adam(self.handle, which, layer, p(mw), p(vw), p(mb), p(vb), C.byref(st) if step else None))
        return mw, vw, mb, vb, (st.value if step else None)

    def load_adam(self, which, layer, m_w=None, v_w=None, m_b=None, v_b=None, step=-1):
        """aae_load_adam: any of the four moment arrays (None = left as it is); step < 0 leaves the count alone."""
        out, inn = self.linear_shape({O_ENC: 0, O_GEN: 0, O_DEC: 1, O_DISC: 2}[which], layer)
        keep = [self._host_in(a, s, n) for a, s, n in ((m_w, (out, inn), "m_w"), (v_w, (out, inn), "v_w"),
                                                      (m_b, (out,), "m_b"), (v_b, (out,), "v_b"))]
        with self._on_device():
            _check(self.lib.aae_load_adam(self.handle, which, layer, keep[0][1], keep[1][1], keep[2][1], keep[3][1], int(step)))

    # ---- batches / randomness ----------------------------------------------------------
    def _batch(self, csr, row_start, n_rows, rows=None, bounded=True):
        b = AaeBatch()
        b.indptr_dev, b.indices_dev, b.values_dev = csr.indptr.data_ptr(), csr.indices.data_ptr(), csr.values.data_ptr()
        b.rows_dev = rows.data_ptr() if rows is not None else None
        b.row_start, b.n_rows = int(row_start), int(n_rows)
        b.nnz_bound = int(n_rows * max(1, csr.nnz_per_row_max))
        if bounded and b.nnz_bound > self.cfg.max_nnz:
            raise ValueError(f"batch may hold {b.nnz_bound} entries but the model was created with max_nnz="
                             f"{self.cfg.max_nnz}")
        b.max_row_nnz = int(csr.nnz_per_row_max)
        # the content id a named-ahead batch is matched by (ABI 3): the matrix's generation and the row ids' (row_ids());
        # 0 - never matched - when either is unknown
        cg = int(getattr(csr, "generation", 0))
        rg = 1 if rows is None else int(getattr(rows, "_aae_generation", 0))
        b.generation = ((cg << 32) ^ rg) & 0x7FFFFFFFFFFFFFFF if cg and rg else 0
        return b

    def _inject(self, masks, z_real):
        # every step-opening entry point passes through here: the buffers kept alive for the PREVIOUS step (condition
        # blocks, injected masks, packets handed to the library by pointer) are released now, whatever the rng mode
        self._keep = []
        if masks is None and z_real is None:
            return None
        inj = AaeRngInject()
        keep = []
        for i in range(12):
            mk = None if masks is None or i >= len(masks) or masks[i] is None else masks[i]
            if mk is not None:
                t = torch.as_tensor(np.ascontiguousarray(mk, dtype=np.uint8), device=self.device) \
                    if not torch.is_tensor(mk) else mk.to(self.device, torch.uint8).contiguous()
                keep.append(t)
                inj.masks_dev[i] = t.data_ptr()
            else:
                inj.masks_dev[i] = None
        if z_real is not None:
            z = torch.as_tensor(np.ascontiguousarray(z_real, dtype=np.float32), device=self.device) \
                if not torch.is_tensor(z_real) else z_real.to(self.device, torch.float32).contiguous()
            keep.append(z)
            inj.z_real_dev = z.data_ptr()
        self._keep = keep
        return inj

    # ---- the step --------------------------------------------------------------------
    def prefetch(self, csr, row_start, n_rows, rows=None):
        """Name the batch of the step AFTER the next one (aae_prefetch_batch): its unique-item list and deferred-Adam
        catch-up run beside the next step.  `rows` (device int32 row ids) must stay alive and unchanged until then."""
        b = self._batch(csr, row_start, n_rows, rows)
        self._pf_keep = (csr, rows)
        _check(self.lib.aae_prefetch_batch(self.handle, C.byref(b)))

    def set_input_noise(self, noise):
        """The NEXT training step's encoder reads the dense batch + `noise` ([rows, n_items] float32, already scaled by
        the noise factor) instead of the sparse rows (aae_set_input_noise; DenoisingAutoEncoder corrupt='gauss')."""
        noise = noise.to(self.device, torch.float32).contiguous()
        assert noise.shape[1] == self.N
        self._noise_keep = noise
        _check(self.lib.aae_set_input_noise(self.handle, _ptr(noise), noise.shape[1]))

    def set_input_noise_gen(self, scale):
        """The NEXT training step's encoder reads the dense batch + `scale` x N(0, 1) drawn from the device generator (stream
        14 of that step, keyed by the global batch row and the item: aae_set_input_noise_gen) - no noise block in memory, and
        `seed` determines the draws.  Replaces a pending set_input_noise, and is replaced by a later one."""
        self._noise_keep = None
        _check(self.lib.aae_set_input_noise_gen(self.handle, float(scale)))

    def dae_thin(self, csr, p, out=None):
        """`csr` with every entry zeroed with probability `p` by the device generator (aae_dae_thin: stream 13 of the NEXT
        training step of this handle, keyed by the row's index in `csr` and the item id): a DeviceCSR that shares csr's
        structure and carries new values - `out` (a float32 device tensor of csr.values' shape; csr.values itself is allowed)
        or a fresh tensor - and a content id of its own."""
        if out is None:
            out = torch.empty_like(csr.values)
        elif out.shape != csr.values.shape or out.dtype != torch.float32 or out.device != csr.values.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous float32 device tensor of csr.values' shape")
        with self._on_device():
            _check(self.lib.aae_dae_thin(self.handle, _ptr(csr.indptr), _ptr(csr.indices), _ptr(csr.values), int(csr.shape[0]),
                                         float(p), _ptr(out), self._stream()))
        thinned = DeviceCSR.__new__(DeviceCSR)
        thinned.touch()                                          # (new values: a content id of its own, aae_batch.generation)
        thinned.shape, thinned.nnz_per_row_max = csr.shape, csr.nnz_per_row_max
        thinned.indptr, thinned.indices, thinned.values = csr.indptr, csr.indices, out
        return thinned

    def step(self, csr, row_start, n_rows, rows=None, cond=None, masks=None, z_real=None):
        """One partial_fit without generic conditions (cond: device tensor [n_rows, cond_inc])."""
        b = self._batch(csr, row_start, n_rows, rows)
        inj = self._inject(masks, z_real)
        if cond is not None:
            cond = upload(cond, self.device, torch.float32).contiguous()
            self._keep.append(cond)
        with self._on_device():
            _check(self.lib.aae_step(self.handle, C.byref(b), _ptr(cond), C.byref(inj) if inj else None,
                                     self._stream()))

    # ---- the ae phase cut at the decoder's output layer (vocabulary-sharded data parallelism) -----------
    def ae_forward(self, csr, row_start, n_rows, rows=None, cond=None, masks=None, z_real=None):
        """Encoder + decoder hidden layers; the last hidden activation stays in tensor(T_ACT_DH2, padded=True)."""
        b = self._batch(csr, row_start, n_rows, rows)
        inj = self._inject(masks, z_real)
        if cond is not None:
            cond = upload(cond, self.device, torch.float32).contiguous()
            self._keep.append(cond)
        with self._on_device():
            _check(self.lib.aae_ae_forward(self.handle, C.byref(b), _ptr(cond), C.byref(inj) if inj else None,
                                           self._stream()))

    def output_layer_step(self, csr=None, row_start=0, n_rows=0, rows=None):
        """The decoder's output layer over this handle's items from T_ACT_DH2 -> dL/d(dh2) in T_ACT_DA2; csr = None
        continues the step ae_forward started on this handle."""
        b = self._batch(csr, row_start, n_rows, rows) if csr is not None else None
        with self._on_device():
            _check(self.lib.aae_output_layer_step(self.handle, C.byref(b) if b is not None else None, self._stream()))

    def ae_backward(self, da2=None):
        """Decoder hidden + encoder backward from dL/d(dh2) (None = this handle's T_ACT_DA2)."""
        if da2 is not None:
            assert da2.is_cuda and da2.dtype == torch.float32 and da2.stride(1) == 1
            self._keep.append(da2)
        with self._on_device():
            _check(self.lib.aae_ae_backward(self.handle, _ptr(da2), da2.stride(0) if da2 is not None else 0,
                                            self._stream()))

    # ---- the first encoder layer sharded over the vocabulary as well (include/aaerec_hip.h: aae_first_layer_*) ------
    def set_doc_l1(self, doc_l1):
        """Slice handle: L1 norms of the complete documents (float32 device tensor indexed by document id; None = the
        batch's own rows are complete)."""
        if doc_l1 is not None:
            assert doc_l1.is_cuda and doc_l1.dtype == torch.float32 and doc_l1.is_contiguous()
        self._doc_l1 = doc_l1                      # (keeps the buffer alive as long as the handle uses it)
        _check(self.lib.aae_set_doc_l1(self.handle, _ptr(doc_l1)))

    def set_first_layer_external(self, on=True):
        """Replica handle: a1_rows() is filled by the caller, dL/d(a1) comes back in ga1_rows(); enc.lin1 stays untouched."""
        _check(self.lib.aae_set_first_layer_external(self.handle, 1 if on else 0))
        self._ext_first = bool(on)

    def ga1_packet(self, n_rows, with_decoder):
        """(flat view, rows part in floats, offset of the small layers' gradient span in floats): dL/d(a1) of the last
        encoder backward and, right behind it in the arena, the gradients of enc.lin1's bias, enc.lin2, enc.lin3 (and
        dec.lin1, dec.lin2 when with_decoder) - ONE contiguous packet for the both-sharded scheme's all-gather.  Export
        mode with an external first layer only (the library keeps dL/d(a1) right-aligned in front of that span)."""
        a, b, e = AaeTensor(), AaeTensor(), AaeTensor()
        _check(self.lib.aae_tensor_info(self.handle, T_ACT_GA1, C.byref(a)))
        _check(self.lib.aae_tensor_info(self.handle, T_GRAD + T_ENC_B1, C.byref(b)))
        _check(self.lib.aae_tensor_info(self.handle, T_GRAD + (T_DEC_V2 if with_decoder else T_ENC_W3), C.byref(e)))
        start = a.byte_offset + (a.rows - n_rows) * a.ld * 4
        end = e.byte_offset + e.rows * e.ld * 4
        assert self._ext_first and start + n_rows * a.ld * 4 <= b.byte_offset < end
        return self.arena[start:end].view(torch.float32), n_rows * a.ld, (b.byte_offset - start) // 4

    def first_layer_forward(self, csr=None, row_start=0, n_rows=0, rows=None, bias=None):
        """This handle's items' share of the first layer's pre-activations -> a1_rows(); csr = None: the running batch
        again with the weights as they are now.  bias: the replicas' enc.lin1 bias (device tensor) on exactly one share."""
        b = self._batch(csr, row_start, n_rows, rows) if csr is not None else None
        with self._on_device():
            _check(self.lib.aae_first_layer_forward(self.handle, C.byref(b) if b is not None else None, _ptr(bias),
                                                    self._stream()))

    def first_layer_update(self, which, ga1=None, rows_per_block=0, block_stride=0):
        """enc.lin1's rows of this handle's items from dL/d(a1) of the running batch, optimiser `which`.  ga1 = None:
        ga1_rows(); else a float32 device tensor holding blocks of `rows_per_block` rows (leading dimension = ga1_rows()'s),
        `block_stride` floats apart (the ranks' packets of an all-gather, read where they landed)."""
        if ga1 is not None:         # (the caller's buffer: it must stay alive until the stream has passed this call)
            assert ga1.is_cuda and ga1.dtype == torch.float32 and ga1.is_contiguous()
        if ga1 is not None and self._ga1_ld is None:
            self._ga1_ld = self.ga1_rows(1).stride(0)
        ld = self._ga1_ld if ga1 is not None else 0
        with self._on_device():
            _check(self.lib.aae_first_layer_update(self.handle, _ptr(ga1), ld, int(rows_per_block), int(block_stride),
                                                   int(which), self._stream()))

    def first_layer_bias(self):
        """enc.lin1's bias as a device view (what one share of first_layer_forward adds)."""
        return self.tensor(T_ENC_B1, padded=True)

    def apply_gathered(self, which_a, which_b, packets, peer_stride, n_peers, span_offset):
        """Optimiser which_a (+ dec_optim's small layers when which_b == O_DEC, else -1) on the replica's small layers
        from the gathered packets (aae_apply_gathered): one launch, the peers summed in rank order inside it."""
        with self._on_device():
            _check(self.lib.aae_apply_gathered(self.handle, int(which_a), int(which_b), _ptr(packets), int(peer_stride),
                                               int(n_peers), int(span_offset), self._stream()))

    def dp_reserve(self, n_rows, world):
        """Set-up for dp_step: the gathered-packet scratch for `world` ranks x n_rows local documents (aae_dp_reserve)."""
        with self._on_device():
            _check(self.lib.aae_dp_reserve(self.handle, int(n_rows), int(world)))

    def dp_step(self, slice_model, coll, csr, row_start, n_rows, slice_csr, g_row_start, global_rows, rows=None, g_rows=None,
                next_global=None, cond=None, masks=None, z_real=None):
        """One data-parallel partial_fit as ONE library call (aae_dp_step): this replica's documents + the global batch in
        the slice model's corpus; every kernel and every collective of the step is enqueued by the library on this
        handle's stream.  coll: an AaeCollectives table (parallel.rccl_collectives / parallel.python_collectives).
        next_global = (row_start, rows) of the NEXT global batch in slice_csr: named ahead to the slice model."""
        b = self._batch(csr, row_start, n_rows, rows)
        g = slice_model._batch(slice_csr, g_row_start, global_rows, g_rows)
        nxt = None
        if next_global is not None:
            nxt = slice_model._batch(slice_csr, next_global[0], global_rows, next_global[1])
            slice_model._pf_keep = (slice_csr, next_global[1])
        inj = self._inject(masks, z_real)
        slice_model._keep = []
        if cond is not None:
            cond = upload(cond, self.device, torch.float32).contiguous()
            self._keep.append(cond)
        self._keep.append((g_rows, rows))
        with self._on_device():
            _check(self.lib.aae_dp_step(self.handle, slice_model.handle, C.byref(coll), C.byref(b), C.byref(g),
                                        C.byref(nxt) if nxt is not None else None, _ptr(cond),
                                        C.byref(inj) if inj else None, self._stream()))

    def shard_step(self, coll, csr, row_start, n_rows, item_share, rows=None, next_rows=None, cond=None, masks=None, z_real=None):
        """One partial_fit of the item-sharded model with replicated hidden stacks as ONE library call (aae_shard_step):
        this handle = an item slice of enc.lin1 / dec.lin3 + a full copy of the hidden layers; the batch is the GLOBAL batch
        in the slice's corpus; three all-reduces of [rows, n_hidden] partial sums through `coll`.  next_rows = (row_start,
        rows, n_rows) of the next global batch (named ahead; rows = device int32 row ids or None)."""
        b = self._batch(csr, row_start, n_rows, rows)
        nxt = None
        if next_rows is not None:
            nxt = self._batch(csr, next_rows[0], next_rows[2], next_rows[1])
            self._pf_keep = (csr, next_rows[1])
        inj = self._inject(masks, z_real)
        if cond is not None:
            cond = upload(cond, self.device, torch.float32).contiguous()
            self._keep.append(cond)
        self._keep.append(rows)
        with self._on_device():
            _check(self.lib.aae_shard_step(self.handle, C.byref(coll), C.byref(b), C.byref(nxt) if nxt is not None else None,
                                           _ptr(cond), C.byref(inj) if inj else None, float(item_share), self._stream()))

    def a1_rows(self, n_rows):
        """[n_rows, ld] view of the first layer's pre-activations."""
        return self.tensor(T_ACT_A1, padded=True)[:n_rows]

    def ga1_rows(self, n_rows):
        """[n_rows, ld] view of dL/d(a1) of the last encoder backward (a replica in export mode with an external first
        layer keeps it in the LAST rows of its buffer: see ga1_packet)."""
        t = self.tensor(T_ACT_GA1, padded=True)
        return t[t.shape[0] - n_rows:] if (self._ext_first and self.cfg.grad_mode == GRAD_EXPORT) else t[:n_rows]

    def dh2_rows(self, n_rows):
        """[n_rows, ld] view of the decoder's last hidden activation (with its bias-input column and padding)."""
        return self.tensor(T_ACT_DH2, padded=True)[:n_rows]

    def da2_rows(self, n_rows):
        """[n_rows, ld] view of dL/d(dh2): written by output_layer_step, read by ae_backward()."""
        return self.tensor(T_ACT_DA2, padded=True)[:n_rows]

    def cond_grad(self, n_rows):
        """dL/d(cond) of the last step's autoencoder phase: [n_rows, cond_inc] view (trainable conditions)."""
        return self.tensor(T_ACT_DZC)[:n_rows, self.c:]

    def ae_encode(self, csr, row_start, n_rows, rows=None, masks=None, z_real=None):
        b = self._batch(csr, row_start, n_rows, rows)
        inj = self._inject(masks, z_real)
        z = torch.empty(n_rows, self.c, dtype=torch.float32, device=self.device)
        with self._on_device():
            _check(self.lib.aae_ae_encode(self.handle, C.byref(b), C.byref(inj) if inj else None, _ptr(z),
                                          self._stream()))
        return z

    def ae_decode_backward(self, zc):
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        assert zc.shape[1] == self.c + self.cond_inc, "conditions.size_increment() mismatch"
        dzc = torch.empty_like(zc)
        with self._on_device():
            _check(self.lib.aae_ae_decode_backward(self.handle, _ptr(zc), zc.shape[1], None, _ptr(dzc), self._stream()))
        return dzc

    def decoder_step(self, csr, row_start, n_rows, zin, rows=None, masks=None, want_grad=True):
        """DecodingRecommender.partial_fit (aae.py:489-517): decoder forward on zin [n_rows, n_code + cond_inc],
        BCE against the CSR rows, decoder backward + optimiser step.  masks: (dec.drop1, dec.drop2) keep-masks
        in rng_mode='inject'.  Returns dL/dzin (device) or None."""
        b = self._batch(csr, row_start, n_rows, rows)
        inj = self._inject([None, None, masks[0], masks[1]] if masks is not None else None, None)
        zin = zin.detach().to(self.device, torch.float32).contiguous()
        assert zin.shape == (n_rows, self.c + self.cond_inc), "decoder input width mismatch"
        dz = torch.empty_like(zin) if want_grad else None
        self._keep.append(zin)
        with self._on_device():
            _check(self.lib.aae_decoder_step(self.handle, C.byref(b), _ptr(zin), zin.shape[1],
                                             C.byref(inj) if inj else None, _ptr(dz), self._stream()))
        return dz

    def vae_step(self, csr, row_start, n_rows, rows=None, cond=None, eps=None):
        """VAE.partial_fit (vae.py:147-186).  eps: [n_rows, n_code] standard-normal draws (rng_mode='inject')."""
        b = self._batch(csr, row_start, n_rows, rows)
        keep = []
        if cond is not None:
            cond = upload(cond, self.device, torch.float32).contiguous(); keep.append(cond)
        if eps is not None:
            eps = torch.as_tensor(eps, dtype=torch.float32).to(self.device).contiguous(); keep.append(eps)
        self._keep = keep
        with self._on_device():
            _check(self.lib.aae_vae_step(self.handle, C.byref(b), _ptr(cond), _ptr(eps), self._stream()))

    def vae_encode(self, csr, row_start, n_rows, rows=None, eps=None, train=True):
        """z [n_rows, n_code] of the VAE's encoder + reparametrisation (aae_vae_encode); train=True opens a step."""
        b = self._batch(csr, row_start, n_rows, rows)
        if eps is not None:
            eps = torch.as_tensor(eps, dtype=torch.float32).to(self.device).contiguous()
        z = torch.empty(n_rows, self.c, dtype=torch.float32, device=self.device)
        self._keep = [eps, z]
        with self._on_device():
            _check(self.lib.aae_vae_encode(self.handle, C.byref(b), _ptr(eps), _ptr(z), int(bool(train)), self._stream()))
        return z

    def vae_decode_backward(self, zc):
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        dzc = torch.empty_like(zc)
        self._keep = self._keep + [zc, dzc]
        with self._on_device():
            _check(self.lib.aae_vae_decode_backward(self.handle, _ptr(zc), zc.shape[1], _ptr(dzc), self._stream()))
        return dzc

    def vae_encoder_backward(self, dz):
        dz = dz.detach().to(self.device, torch.float32).contiguous()
        self._keep = self._keep + [dz]
        with self._on_device():
            _check(self.lib.aae_vae_encoder_backward(self.handle, _ptr(dz), dz.shape[1], self._stream()))

    def vae_predict(self, csr, row_start, n_rows, cond=None, eps=None):
        b = self._batch(csr, row_start, n_rows)
        out = self._out_buffer(n_rows)
        if cond is not None:
            cond = upload(cond, self.device, torch.float32).contiguous()
        if eps is not None:
            eps = torch.as_tensor(eps, dtype=torch.float32).to(self.device).contiguous()
        with self._on_device():
            _check(self.lib.aae_vae_predict(self.handle, C.byref(b), _ptr(cond), _ptr(eps), _ptr(out), out.shape[1],
                                            self._stream()))
        return out[:, :self.N]

    def ae_encoder_backward(self, dz):
        dz = dz.detach().to(self.device, torch.float32).contiguous()
        self._keep.append(dz)
        with self._on_device():
            _check(self.lib.aae_ae_encoder_backward(self.handle, _ptr(dz), dz.shape[1], self._stream()))

    def disc_gen(self):
        with self._on_device():
            _check(self.lib.aae_disc_gen(self.handle, None, self._stream()))

    def disc_step(self):
        with self._on_device():
            _check(self.lib.aae_disc_step(self.handle, None, self._stream()))

    def gen_step(self):
        with self._on_device():
            _check(self.lib.aae_gen_step(self.handle, None, self._stream()))

    def apply_updates(self, which, skip=-1):
        with self._on_device():
            _check(self.lib.aae_apply_updates_except(self.handle, which, skip, self._stream()))

    def apply_shard(self, tid, row_begin, row_end, grad_shard, which):
        self._keep.append(grad_shard)
        with self._on_device():
            _check(self.lib.aae_apply_shard(self.handle, tid, row_begin, row_end, C.c_void_p(grad_shard.data_ptr()),
                                            which, self._stream()))

    big_tensor_id = T_DEC_V3      # the decoder's output layer: the one tensor worth sharding across ranks

    def big_grad(self):
        """(tensor id, padded gradient view [rows, ld], padded parameter view [rows, ld]) of the one
        tensor worth sharding across data-parallel ranks: the decoder's output layer."""
        return T_DEC_V3, self.tensor(T_GRAD + T_DEC_V3, padded=True), self.tensor(T_DEC_V3, padded=True)

    def _w1_layout(self, cap):
        """(rows, header words, total floats) of a packet with room for `cap` rows (None = the model's w1_cap)."""
        if self._w1_packet is None:
            hw, tot = C.c_int64(), C.c_int64()
            _check(self.lib.aae_w1_packet_floats(self.handle, self.w1_cap, C.byref(hw), C.byref(tot)))
            assert hw.value == self._w1_hdr
            self._w1_small = tot.value - hw.value - self.w1_cap * self.h
            self._w1_packet = torch.zeros(tot.value, dtype=torch.float32, device=self.device)
        cap = self.w1_cap if cap is None else max(1, min(int(cap), self.w1_cap))
        hdr = (1 + cap + 3) & ~3
        return cap, hdr, hdr + cap * self.h + self._w1_small

    def w1_export(self, cap=None):
        """Pack this rank's first-layer gradient rows: one flat float32 tensor = int32 header (count, item ids) +
        rows [cap, n_hidden] + the encoder's small-layer gradients.  cap: an upper bound on the distinct items of
        this exchange that every rank agrees on (e.g. the largest entry count of any rank's share of the batch);
        the default is the model-wide worst case w1_cap - the packet is what the all-gather moves."""
        cap, hdr, total = self._w1_layout(cap)
        pk = self._w1_packet[:total]
        with self._on_device():
            _check(self.lib.aae_w1_export(self.handle, C.c_void_p(pk.data_ptr()), C.c_void_p(pk.data_ptr() + 4 * hdr), cap,
                                          self._stream()))
        return pk

    def w1_import(self, packets, n_peers, which, cap=None, stride_floats=None):
        """Sum the peers' packed rows (flat tensor of n_peers packets of w1_export(cap)) and run optimiser `which`.
        stride_floats: distance between consecutive peers' packets when they carry riders behind them."""
        cap, hdr, total = self._w1_layout(cap)
        stride = total if stride_floats is None else int(stride_floats)
        assert stride >= total and packets.numel() >= (n_peers - 1) * stride + total
        self._keep.append(packets)
        with self._on_device():
            _check(self.lib.aae_w1_import(self.handle, C.c_void_p(packets.data_ptr()),
                                          C.c_void_p(packets.data_ptr() + 4 * hdr), cap, n_peers, 4 * stride, which,
                                          self._stream()))

    def set_rng_rows(self, row_offset, global_rows):
        """Device RNG under data parallelism: this rank's rows are [row_offset, row_offset + n_rows) of a global batch
        of global_rows; with one seed on every rank the ranks draw what a single process draws for the whole batch."""
        _check(self.lib.aae_set_rng_rows(self.handle, int(row_offset), int(global_rows)))

    def set_grad_scale(self, scale):
        _check(self.lib.aae_set_grad_scale(self.handle, float(scale)))

    def profile_enable(self, on=True, kernels=None):
        """kernels: iterable of kernel ids to time (None = all)."""
        if on and kernels is not None:
            on = sum(1 << (k + 1) for k in kernels)
        _check(self.lib.aae_profile_enable(self.handle, int(on)))

    def profile_read(self, kernel_id):
        """(total_ms, launches) of the hipEvent pairs recorded around `kernel_id` since the last read."""
        ms, n = C.c_double(), C.c_int64()
        _check(self.lib.aae_profile_read(self.handle, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def losses(self):
        out = (C.c_float * 3)()
        with self._on_device():
            _check(self.lib.aae_read_losses(self.handle, C.byref(out), self._stream()))
        return float(out[0]), float(out[1]), float(out[2])

    # ---- predict ------------------------------------------------------------------------
    def _out_buffer(self, n_rows):
        ld = (self.N + 3) & ~3
        return torch.empty(n_rows, ld, dtype=torch.float32, device=self.device)

    def predict(self, csr, row_start, n_rows, cond=None):
        b = self._batch(csr, row_start, n_rows)
        out = self._out_buffer(n_rows)
        if cond is not None:
            cond = upload(cond, self.device, torch.float32).contiguous()
        with self._on_device():
            _check(self.lib.aae_predict(self.handle, C.byref(b), _ptr(cond), _ptr(out), out.shape[1], self._stream()))
        return out[:, :self.N]

    def rank_max_rows(self, k=10):
        """Rows one predict_topk / decode_topk call may rank (aae_rank_max_rows): far more than max_batch where the fused
        predict -> rank kernels apply, max_batch otherwise."""
        return self._max_rows(int(k), self.lib.aae_rank_max_rows, int(k))

    def _max_rows(self, key, entry, *args):
        """A row limit of the handle (one of the *_max_rows entry points), asked once."""
        if key not in self._rank_rows:
            out = C.c_int32()
            _check(entry(self.handle, *args, C.byref(out)))
            self._rank_rows[key] = int(out.value)
        return self._rank_rows[key]

    def rank_long_stats(self):
        """The fused k > 32 ranking calls since the last read (aae_rank_long_stats): calls, rows, rows whose collect list
        overflowed, entries collected, the most entries of any row.  Resets the counters."""
        out = (C.c_int64 * 5)()
        _check(self.lib.aae_rank_long_stats(self.handle, out))
        return dict(zip(("calls", "rows", "overflow_rows", "entries", "max_entries"), (int(v) for v in out)))

    def predict_topk(self, csr, row_start, n_rows, k, cond=None, exclude_known=True):
        """(ids int32 [n_rows, k], scaled scores float32 [n_rows, k]) - device tensors.  n_rows <= rank_max_rows(k),
        1 <= k <= RANK_K_MAX (k > 32: the long-list kernels, csrc/rank_long.h; equal logits go to the smaller item id).
        Ties: the reference leaves items of equal fp32 score in np.argpartition's order (evaluation.py:20-58).  Calls within
        the fused path's row limit order such items by their LOGIT (saturated sigmoids included), the dense fallback by the
        smaller item id: the k scores are the same either way, the items named may differ exactly where scores tie
        (tests/test_rank_gpu.py::test_saturated_scores_tie_and_both_rank_paths_return_a_valid_top_k)."""
        return self._topk(self.lib.aae_predict_topk, csr, row_start, n_rows, k, exclude_known, (self._cond_rows(cond),))

    def _cond_rows(self, cond):
        return None if cond is None else upload(cond, self.device, torch.float32).contiguous()

    def _lead(self, batch, lo, hi, per_row, zc):
        """The arguments of a ranking entry point from the handle to the batch for rows [lo, hi) of a call: the predict form
        (handle, batch, the rows of cond / eps) or, with zc, the decode form (handle, the rows of zc, its stride, batch)."""
        if zc is not None:
            return (self.handle, zc[lo:hi], zc.shape[1], batch)
        return (self.handle, batch, *(None if t is None else t[lo:hi] for t in per_row))

    def _topk(self, entry, csr, row_start, n_rows, k, exclude_known, per_row=(), zc=None):
        """A list call of the handle (per_row, zc: _lead)."""
        # (beyond max_batch: the fused rank path, which has no per-batch lists)
        b = self._batch(csr, row_start, n_rows, bounded=n_rows <= self.max_batch)
        return _list_call(entry, self.device, self._on_device(), n_rows, k, exclude_known, self._lead(b, 0, n_rows, per_row, zc))

    def _ranks(self, entry, cap, csr, row_start, n_rows, truth_csr, exclude_known, per_row=(), zc=None):
        """A full-ranking call of the handle over any number of rows, `cap` (the entry's row limit) at a time, every chunk with
        its rows of per_row / zc (_lead).  A chunk without truth entries builds no batch and calls nothing."""
        out = []
        for s0 in range(row_start, row_start + n_rows, cap):
            n, lo = min(cap, row_start + n_rows - s0), s0 - row_start
            nnz, tb = self._truth_span(truth_csr, s0, n)
            lead = ()
            if nnz:
                lead = self._lead(self._batch(csr, s0, n, bounded=n <= self.max_batch), lo, lo + n, per_row, zc) + (tb,)
            out.append(_ranks_call(entry, self.device, self._on_device(), nnz, exclude_known, lead))
        return torch.cat(out) if len(out) != 1 else out[0]

    def decode_topk(self, zc, csr, row_start, k, exclude_known=True):
        """Top-k of decode(zc) for the input rows csr[row_start : row_start + len(zc)] (aae_decode_topk)."""
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        return self._topk(self.lib.aae_decode_topk, csr, row_start, zc.shape[0], k, exclude_known, zc=zc)

    # ---- full ranking: the rank of every held-out item (csrc/rank_full.h) ------------------------
    def rank_full_max_rows(self):
        """Rows one aae_predict_ranks / aae_decode_ranks call may take (aae_rank_full_max_rows)."""
        return self._max_rows("full", self.lib.aae_rank_full_max_rows)

    def _truth_span(self, truth_csr, row_start, n_rows):
        """(entries of truth rows [row_start, row_start + n_rows), the batch naming them); indptr is read on the host once."""
        gen, ip = getattr(truth_csr, "_indptr_host", (None, None))
        if ip is None or gen != getattr(truth_csr, "generation", 0):
            gen, ip = getattr(truth_csr, "generation", 0), truth_csr.indptr.cpu().numpy()
            truth_csr._indptr_host = (gen, ip)
        if truth_csr.shape[1] != self.N:
            raise ValueError(f"the ground truth has {truth_csr.shape[1]} columns, the model {self.N} items")
        return int(ip[row_start + n_rows] - ip[row_start]), self._batch(truth_csr, row_start, n_rows, bounded=False)

    def predict_ranks(self, csr, row_start, n_rows, truth_csr, cond=None, exclude_known=True):
        """int32 device tensor: for every stored entry of truth_csr[row_start : row_start + n_rows], in CSR order, the
        1-based rank of that item among its row's items in predict_topk's ordering (known items excluded from the ranking
        with exclude_known; better score first, equal logits to the smaller id; a truth item that is itself a known item
        ranks behind every rankable one: n_rankable + 1 + #{known ids < it}).  Any number of rows: chunked by
        rank_full_max_rows().  Row i of truth_csr belongs to row i of csr."""
        return self._ranks(self.lib.aae_predict_ranks, self.rank_full_max_rows(), csr, row_start, n_rows, truth_csr, exclude_known,
                           (self._cond_rows(cond),))

    def decode_ranks(self, zc, csr, row_start, truth_csr, exclude_known=True):
        """The same for decode(zc): the input rows csr[row_start : row_start + len(zc)] (aae_decode_ranks)."""
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        return self._ranks(self.lib.aae_decode_ranks, self.rank_full_max_rows(), csr, row_start, zc.shape[0], truth_csr,
                           exclude_known, zc=zc)

    # ---- the VAE's predict -> rank (aae_vae_predict_topk / ...; csrc/abi_rank.h, the VAE's form) ----------
    def vae_rank_max_rows(self, k=10):
        """Rows one vae_predict_topk / vae_decode_topk call may rank (aae_vae_rank_max_rows)."""
        return self._max_rows(("vae", int(k)), self.lib.aae_vae_rank_max_rows, int(k))

    def vae_rank_full_max_rows(self):
        """Rows one aae_vae_predict_ranks / aae_vae_decode_ranks call may take (aae_vae_rank_full_max_rows)."""
        return self._max_rows("vae_full", self.lib.aae_vae_rank_full_max_rows)

    def _eps_rows(self, eps, n_rows):
        if eps is None:
            return None
        eps = torch.as_tensor(eps, dtype=torch.float32).to(self.device).contiguous()
        if tuple(eps.shape) != (n_rows, self.c):
            raise ValueError(f"eps has shape {tuple(eps.shape)}, the call {(n_rows, self.c)}: one row of draws per row")
        return eps

    def vae_predict_topk(self, csr, row_start, n_rows, k, cond=None, eps=None, exclude_known=True):
        """predict_topk of a VAE handle: the scores of vae_predict for the same rows and eps ([n_rows, n_code]; None: the
        device generator), ranked as predict_topk ranks.  n_rows <= vae_rank_max_rows(k)."""
        return self._topk(self.lib.aae_vae_predict_topk, csr, row_start, n_rows, k, exclude_known,
                          (self._cond_rows(cond), self._eps_rows(eps, n_rows)))

    def vae_decode_topk(self, zc, csr, row_start, k, exclude_known=True):
        """Top-k of the VAE's decode(zc) for the input rows csr[row_start : row_start + len(zc)] (aae_vae_decode_topk)."""
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        return self._topk(self.lib.aae_vae_decode_topk, csr, row_start, zc.shape[0], k, exclude_known, zc=zc)

    def vae_predict_ranks(self, csr, row_start, n_rows, truth_csr, cond=None, eps=None, exclude_known=True):
        """predict_ranks of a VAE handle (aae_vae_predict_ranks).  Any number of rows: chunked by vae_rank_full_max_rows(),
        every chunk with its rows of cond and eps."""
        return self._ranks(self.lib.aae_vae_predict_ranks, self.vae_rank_full_max_rows(), csr, row_start, n_rows, truth_csr,
                           exclude_known, (self._cond_rows(cond), self._eps_rows(eps, n_rows)))

    def vae_decode_ranks(self, zc, csr, row_start, truth_csr, exclude_known=True):
        """The same for the VAE's decode(zc) (aae_vae_decode_ranks)."""
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        return self._ranks(self.lib.aae_vae_decode_ranks, self.vae_rank_full_max_rows(), csr, row_start, zc.shape[0], truth_csr,
                           exclude_known, zc=zc)

    # ---- the held-out loss: per-row sums on the device, no score matrix (csrc/loss_eval.h) ----------------
    def loss_max_rows(self):
        """Rows one predict_loss / decode_loss call (a VAE handle: vae_predict_loss / vae_decode_loss) may take."""
        if self.vae:
            return self._max_rows("vae_loss", self.lib.aae_vae_loss_max_rows)
        return self._max_rows("loss", self.lib.aae_loss_max_rows)

    def _loss(self, entry, name, csr, row_start, n_rows, targets, per_row=(), zc=None, mid=(), n_out=1):
        """A loss call of the handle: n_out float64 device tensors [n_rows].  targets: a DeviceCSR of csr's shape (None: csr)."""
        if targets is not None and tuple(targets.shape) != tuple(csr.shape):
            raise ValueError(f"{name}: targets has shape {tuple(targets.shape)}, the input rows {tuple(csr.shape)}")
        b = self._batch(csr, row_start, n_rows, bounded=n_rows <= self.max_batch)
        t = None if targets is None else self._batch(targets, row_start, n_rows, bounded=False)
        outs = tuple(torch.empty(n_rows, dtype=torch.float64, device=self.device) for _ in range(n_out))
        with self._on_device():
            _check(entry(*map(_arg, self._lead(b, 0, n_rows, per_row, zc)), *mid, None if t is None else C.byref(t),
                         *map(_ptr, outs), self._stream()))
        return outs if n_out > 1 else outs[0]

    def predict_loss(self, csr, row_start, n_rows, cond=None, targets=None):
        """float64 device tensor [n_rows]: per row the BCE of predict() against `targets` (None: the input rows), SUMMED over
        the items (aae_predict_loss).  Eval mode; nothing is copied to the host.  n_rows <= loss_max_rows()."""
        return self._loss(self.lib.aae_predict_loss, "predict_loss", csr, row_start, n_rows, targets, (self._cond_rows(cond),))

    def decode_loss(self, zc, csr, row_start, targets=None):
        """The same for decode(zc): the input rows csr[row_start : row_start + len(zc)] (aae_decode_loss)."""
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        return self._loss(self.lib.aae_decode_loss, "decode_loss", csr, row_start, zc.shape[0], targets, zc=zc)

    def vae_predict_loss(self, csr, row_start, n_rows, cond=None, eps=None, row0=0, targets=None):
        """(row_bce, row_kl) float64 device tensors [n_rows] of a VAE handle (aae_vae_predict_loss): the BCE sums of
        vae_predict for the same rows and eps ([n_rows, n_code]; None: the device generator, whose rows count from row0)
        and the rows' KL terms."""
        return self._loss(self.lib.aae_vae_predict_loss, "vae_predict_loss", csr, row_start, n_rows, targets,
                          (self._cond_rows(cond), self._eps_rows(eps, n_rows)), mid=(C.c_int64(int(row0)),), n_out=2)

    def vae_decode_loss(self, zc, csr, row_start, targets=None):
        """The BCE sums of the VAE's decode(zc) (aae_vae_decode_loss)."""
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        return self._loss(self.lib.aae_vae_decode_loss, "vae_decode_loss", csr, row_start, zc.shape[0], targets, zc=zc)

    def encode(self, csr, row_start, n_rows):
        b = self._batch(csr, row_start, n_rows)
        z = torch.empty(n_rows, self.c, dtype=torch.float32, device=self.device)
        with self._on_device():
            _check(self.lib.aae_encode(self.handle, C.byref(b), _ptr(z), self._stream()))
        return z

    def decode(self, zc):
        zc = zc.detach().to(self.device, torch.float32).contiguous()
        out = self._out_buffer(zc.shape[0])
        with self._on_device():
            _check(self.lib.aae_decode(self.handle, _ptr(zc), zc.shape[1], zc.shape[0], _ptr(out), out.shape[1],
                                       self._stream()))
        return out[:, :self.N]
