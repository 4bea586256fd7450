// predict (aae.py:840-870): encode, decode, predict, on-device top-k.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

extern "C" {

// ---- predict (aae.py:840-870) -----------------------------------------------------------
int aae_encode(aae_handle m, const aae_batch* batch, float* z_out, void* stream) {
    if (!m) return fail(AAE_EINVAL, "handle is NULL");
    TRY(set_batch(m, batch));
    hipStream_t s = S(stream);
    TRY(join_deferred(m, s));
    if (m->lazy) TRY(lazy_prepare(m, 0, true, s));
    if (m->use_chain) {
        TRY(gather_first_layer(m, false, nullptr, 0, s));
        ChainBuilder cb(m, m->rows);
        chain_encoder_tail(m, cb, false, nullptr, 0, m->rows, nullptr, s);
        ChainOp& f = cb.add(cop(COP_FINAL_FWD, 2, 2, m->c)); f.aux = m->cfg.enc_final; cop_out(f, m->zc.p, m->ldc);
        if (z_out) { f.out2 = z_out; f.ldo2 = m->c; }
        TRY(launch_chain(m, cb, s));
        m->phase = 0;
        return AAE_OK;
    }
    TRY(encoder_forward(m, false, nullptr, nullptr, 0, 0, false, m->zc.p, m->ldc, s));
    if (z_out) {
        hipLaunchKernelGGL(copy2d_kernel, dim3(grid1d((size_t)m->rows * m->c)), dim3(256), 0, s, m->zc.p, m->ldc,
                           z_out, m->c, m->rows, m->c, 1.0f);
        LAUNCHCHK("copy z");
    }
    m->phase = 0;
    return AAE_OK;
}

}  // extern "C"
namespace {
// the decoder's hidden layers of the rows staged in zc -> m->dh2, eval mode
int dec_hidden_rows(aae_model* m, int n_rows, hipStream_t s) {
    if (m->vae) return vae_dec_hidden(m, n_rows, s);       // (VAE: one hidden layer, fc3)
    if (m->use_chain) return chain_dec_hidden(m, false, n_rows, s);
    return decoder_hidden_forward(m, false, nullptr, nullptr, n_rows, s);
}
}  // namespace
extern "C" {

int aae_decode(aae_handle m, const float* zc_dev, int64_t zc_ld, int32_t n_rows, float* out_dev, int64_t out_ld,
               void* stream) {
    if (!m || !out_dev) return fail(AAE_EINVAL, "handle/out is NULL");
    if (n_rows < 1 || n_rows > m->R) return fail(AAE_EINVAL, "n_rows outside [1, max_batch]");
    if (out_ld < m->N || (out_ld & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        return fail(AAE_EINVAL, "out_dev must be 16-byte aligned with out_ld >= n_items and out_ld % 4 == 0");
    hipStream_t s = S(stream);
    TRY(join_deferred(m, s));
    if (zc_dev) TRY(stage_zc(m, zc_dev, zc_ld, n_rows, s));
    TRY(dec_hidden_rows(m, n_rows, s));
    EpiSigmoid e; e.out = out_dev; e.ld = (int)out_ld;
    TRY(linear_fwd(m->dh2.p, m->ldh, n_rows, m->P[P_V3], e, s, gmode(m)));
    return AAE_OK;
}

int aae_predict(aae_handle m, const aae_batch* batch, const float* cond_dev, float* out_dev, int64_t out_ld,
                void* stream) {
    if (!m) return fail(AAE_EINVAL, "handle is NULL");
    if (m->cfg.cond_inc > 0 && !cond_dev) return fail(AAE_EINVAL, "cond_inc > 0 needs cond_dev");
    TRY(aae_encode(m, batch, nullptr, stream));
    if (m->cfg.cond_inc > 0) {
        hipLaunchKernelGGL(copy2d_kernel, dim3(grid1d((size_t)m->rows * m->cfg.cond_inc)), dim3(256), 0, S(stream),
                           cond_dev, m->cfg.cond_inc, m->zc.p + m->c, m->ldc, m->rows, m->cfg.cond_inc, 1.0f);
        LAUNCHCHK("copy cond");
    }
    return aae_decode(m, nullptr, 0, m->rows, out_dev, out_ld, stream);
}

// predict + on-device remove_non_missing / argtopk (evaluation.py:183-199, 20-58): only the k best
// items per row (ids and min-max-scaled scores) leave the GPU
}  // extern "C"
namespace {
// the [rows][N] scores in the scratch -> [rows][k]: register lists up to k = 32 (kernels.h), the long-list kernel beyond
int topk_from_scores(aae_model* m, int k, int exclude_known, int32_t* idx_out_dev, float* val_out_dev, hipStream_t s) {
    if (rank_long(k)) return rank_long_dense(m, k, exclude_known, idx_out_dev, val_out_dev, s);
    const TopkRowsKernel kernel = pick_topk_rows(rank_K(k));
    if (!kernel) return fail(AAE_ESTATE, "no topk_rows kernel is compiled for this list size");
    hipLaunchKernelGGL(kernel, dim3(m->rows), dim3(256), 0, s, m->G.p, m->ldn, m->N, m->bv, exclude_known, k,
                       reinterpret_cast<int*>(idx_out_dev), val_out_dev);
    LAUNCHCHK("topk_rows");
    return AAE_OK;
}
// the dense form's scores: the rows of `in` (<= max_batch) into the [max_batch][n_items] scratch
int scores_to_scratch(aae_model* m, const RankInput& in, void* stream) {
    if (in.zc) {
        TRY(set_batch(m, &in.batch));
        return aae_decode(m, in.zc, in.zc_ld, m->rows, m->G.p, m->ldn, stream);
    }
    if (in.vae) return aae_vae_predict(m, &in.batch, in.cond, in.eps, m->G.p, m->ldn, stream);
    return aae_predict(m, &in.batch, in.cond, m->G.p, m->ldn, stream);
}
// The ranking calls of a model, either family (in.vae), either form (in.zc): lists ...
int model_topk(aae_model* m, const RankInput& in, int k, int exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    hipStream_t s = S(stream);
    const int rows = in.batch.n_rows;
    if (rows >= 1 && rows <= rank_rows_cap(m, k, in.vae)) {      // fused: no [rows][N] matrix (abi_rank.h)
        const RankWs w = rank_ws(m, rows, k, false);
        m->phase = 0;
        TRY(rank_hidden(m, in, w, s));
        TRY(rank_from_dh2(m, w.p, rank_view(&in.batch), k, exclude_known, idx_out_dev, val_out_dev, s));
        if (!rank_long(k)) return AAE_OK;
        std::vector<std::pair<int, int>> spans;        // rows whose collect list overflowed: through the score matrix
        TRY(rank_long_overflow(m, &in.batch, w.p, s, spans));
        for (const auto& sp : spans) {
            const RankInput sub = rank_cut(m, in, sp.first, sp.second);
            const size_t out0 = (size_t)sp.first * k;
            if (in.vae) TRY(vae_span_scores(m, sub, s));      // (the fused call's own program again: its bits)
            else TRY(scores_to_scratch(m, sub, stream));
            TRY(rank_long_dense(m, k, exclude_known, idx_out_dev + out0, val_out_dev + out0, s));
        }
        return AAE_OK;
    }
    TRY(scores_to_scratch(m, in, stream));
    TRY(topk_from_scores(m, k, exclude_known, idx_out_dev, val_out_dev, s));
    m->phase = 0;
    return AAE_OK;
}
// ... and the rank of every held-out item in the full ranking of its row (rank_full.h)
int model_ranks(aae_model* m, const RankInput& in, const aae_batch* truth, int exclude_known, int32_t* ranks_out_dev, void* stream) {
    hipStream_t s = S(stream);
    const int rows = in.batch.n_rows;
    if (rows >= 1 && rows <= rank_full_rows_cap(m, in.vae)) {      // fused: no [rows][N] matrix (abi_rank.h)
        const RankWs w = rank_ws(m, rows, 32, true);
        m->phase = 0;
        TRY(rank_hidden(m, in, w, s));
        return rank_full_from_dh2(m, w.p, rank_view(&in.batch), rank_view(truth), truth->max_row_nnz, exclude_known, ranks_out_dev, s);
    }
    TRY(scores_to_scratch(m, in, stream));
    TRY(rank_full_dense(m, rank_view(&in.batch), rank_view(truth), exclude_known, ranks_out_dev, s));
    m->phase = 0;
    return AAE_OK;
}
// ---- the held-out loss (loss_eval.h) ----
// the dense form's LOGITS: the rows of `in` (<= max_batch) into the [max_batch][n_items] scratch - the hidden halves of
// aae_predict / aae_vae_predict / aae_decode, then the output layer with a plain store (a VAE handle's [mu | logvar] are
// in m->mulv behind the predict form)
int logits_to_scratch(aae_model* m, const RankInput& in, void* stream) {
    hipStream_t s = S(stream);
    if (in.zc) {
        TRY(set_batch(m, &in.batch));
        TRY(join_deferred(m, s));
        TRY(stage_zc(m, in.zc, in.zc_ld, m->rows, s));
        TRY(dec_hidden_rows(m, m->rows, s));
    } else if (in.vae) {
        TRY(set_batch(m, &in.batch));
        TRY(join_deferred(m, s));
        if (m->lazy) TRY(lazy_prepare(m, 0, true, s));
        TRY(gather_first_layer(m, false, nullptr, 0, s));
        TRY(vae_forward(m, in.cond, in.eps, m->rows, s, in.grow0));
    } else {
        TRY(aae_encode(m, &in.batch, nullptr, stream));
        if (m->cfg.cond_inc > 0) {
            hipLaunchKernelGGL(copy2d_kernel, dim3(grid1d((size_t)m->rows * m->cfg.cond_inc)), dim3(256), 0, s,
                               in.cond, m->cfg.cond_inc, m->zc.p + m->c, m->ldc, m->rows, m->cfg.cond_inc, 1.0f);
            LAUNCHCHK("copy cond");
        }
        TRY(dec_hidden_rows(m, m->rows, s));
    }
    EpiStore e; e.out = m->G.p; e.ld = m->ldn;
    return linear_fwd(m->dh2.p, m->ldh, m->rows, m->P[P_V3], e, s, gmode(m));
}
// ... the loss of the rows of `in` against the rows of `targets`: row_bce [rows] (the sum over the items), and row_kl [rows]
// where it is asked for (a VAE handle's predict form).  Fused or dense by the rule of model_ranks.
int model_loss(aae_model* m, const RankInput& in, const aae_batch* targets, double* row_bce_out, double* row_kl_out, void* stream) {
    hipStream_t s = S(stream);
    const int rows = in.batch.n_rows;
    const BatchView tv = rank_view(targets);
    if (rows >= 1 && rows <= rank_loss_rows_cap(m, in.vae)) {      // fused: no [rows][N] matrix (abi_rank.h)
        const RankWs w = rank_ws(m, rows, 32, kPlanLoss);
        m->phase = 0;
        TRY(rank_hidden(m, in, w, s));
        TRY(loss_from_dh2(m, w.p, tv, targets->max_row_nnz, row_bce_out, s));
        if (row_kl_out) TRY(loss_kl_rows(w.p.mulv, 2 * m->c, m->c, rows, row_kl_out, s));
        return AAE_OK;
    }
    TRY(logits_to_scratch(m, in, stream));
    TRY(loss_rows_dense(m, tv, row_bce_out, s));
    if (row_kl_out) TRY(loss_kl_rows(m->mulv.p, (int)m->mulv.ld, m->c, rows, row_kl_out, s));
    m->phase = 0;
    return AAE_OK;
}
int loss_max_rows(const aae_model* m, bool vae) { return std::max(m->R, rank_loss_rows_cap(m, vae)); }
// the check of the four loss entry points: rank_check_call's for the form, then the targets (NULL: the input rows themselves)
// and the row limit.  Nothing is launched before it passes.
int loss_check_call(const char* who, const aae_model* m, bool vae, int form, bool ptrs, const float* cond_dev, const float* eps_dev,
                    int64_t zc_ld, const aae_batch* batch, const aae_batch*& targets) {
    const int32_t k1 = 1;       // (a list size that passes for every model: a loss call has none)
    TRY(rank_check_call(who, m, vae, form, ptrs, &k1, cond_dev, eps_dev, zc_ld, batch, nullptr));
    const std::string w(who);
    if (!targets) targets = batch;
    if (!targets->indptr_dev || !targets->indices_dev || !targets->values_dev) return fail(AAE_EINVAL, w + ": targets pointers are NULL");
    if (targets->n_rows != batch->n_rows) return fail(AAE_EINVAL, w + ": targets names another number of rows than the call's input rows");
    if (batch->n_rows < 1 || batch->n_rows > loss_max_rows(m, vae))
        return fail(AAE_EINVAL, w + ": n_rows outside [1, " + (vae ? "aae_vae_loss_max_rows" : "aae_loss_max_rows") + "]");
    return AAE_OK;
}
// an entry point's rows: the predict form (cond, eps) or the decode form (zc); grow0: the generator row of the call's first
// row (the ranking calls: 0)
RankInput rank_input(bool vae, const aae_batch* batch, const float* cond_dev, const float* eps_dev, const float* zc_dev, int64_t zc_ld,
                     int grow0 = 0) {
    return RankInput{*batch, cond_dev, eps_dev, zc_dev, zc_ld, grow0, vae};
}
}  // namespace
extern "C" {

int aae_predict_topk(aae_handle m, const aae_batch* batch, const float* cond_dev, int32_t k, int32_t exclude_known,
                     int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    TRY(rank_check_call("aae_predict_topk", m, false, kRankFormPredict, idx_out_dev && val_out_dev, &k, cond_dev, nullptr, 0, batch, nullptr));
    return model_topk(m, rank_input(false, batch, cond_dev, nullptr, nullptr, 0), k, exclude_known, idx_out_dev, val_out_dev, stream);
}

int aae_decode_topk(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, int32_t k,
                    int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    TRY(rank_check_call("aae_decode_topk", m, false, kRankFormDecode, zc_dev && idx_out_dev && val_out_dev, &k, nullptr, nullptr, zc_ld, batch, nullptr));
    return model_topk(m, rank_input(false, batch, nullptr, nullptr, zc_dev, zc_ld), k, exclude_known, idx_out_dev, val_out_dev, stream);
}

int aae_predict_ranks(aae_handle m, const aae_batch* batch, const float* cond_dev, const aae_batch* truth, int32_t exclude_known,
                      int32_t* ranks_out_dev, void* stream) {
    TRY(rank_check_call("aae_predict_ranks", m, false, kRankFormPredict, ranks_out_dev, nullptr, cond_dev, nullptr, 0, batch, truth));
    return model_ranks(m, rank_input(false, batch, cond_dev, nullptr, nullptr, 0), truth, exclude_known, ranks_out_dev, stream);
}

int aae_decode_ranks(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* truth,
                     int32_t exclude_known, int32_t* ranks_out_dev, void* stream) {
    TRY(rank_check_call("aae_decode_ranks", m, false, kRankFormDecode, zc_dev && ranks_out_dev, nullptr, nullptr, nullptr, zc_ld, batch, truth));
    return model_ranks(m, rank_input(false, batch, nullptr, nullptr, zc_dev, zc_ld), truth, exclude_known, ranks_out_dev, stream);
}

int aae_rank_max_rows(aae_handle m, int32_t k, int32_t* rows_out) {
    TRY(rank_check_call("aae_rank_max_rows", m, false, kRankFormRows, rows_out, &k, nullptr, nullptr, 0, nullptr, nullptr));
    *rows_out = std::max(m->R, rank_rows_cap(m, k, false));
    return AAE_OK;
}

int aae_rank_full_max_rows(aae_handle m, int32_t* rows_out) {
    TRY(rank_check_call("aae_rank_full_max_rows", m, false, kRankFormRows, rows_out, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
    *rows_out = std::max(m->R, rank_full_rows_cap(m, false));
    return AAE_OK;
}

// ---- the held-out loss: per row the BCE summed over the items (and the VAE's KL), no score matrix (loss_eval.h) ----
int aae_predict_loss(aae_handle m, const aae_batch* batch, const float* cond_dev, const aae_batch* targets, double* row_bce_dev,
                     void* stream) {
    TRY(loss_check_call("aae_predict_loss", m, false, kRankFormPredict, row_bce_dev, cond_dev, nullptr, 0, batch, targets));
    return model_loss(m, rank_input(false, batch, cond_dev, nullptr, nullptr, 0), targets, row_bce_dev, nullptr, stream);
}

int aae_decode_loss(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* targets,
                    double* row_bce_dev, void* stream) {
    TRY(loss_check_call("aae_decode_loss", m, false, kRankFormDecode, zc_dev && row_bce_dev, nullptr, nullptr, zc_ld, batch, targets));
    return model_loss(m, rank_input(false, batch, nullptr, nullptr, zc_dev, zc_ld), targets, row_bce_dev, nullptr, stream);
}

int aae_vae_predict_loss(aae_handle m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, int64_t row0,
                         const aae_batch* targets, double* row_bce_dev, double* row_kl_dev, void* stream) {
    TRY(loss_check_call("aae_vae_predict_loss", m, true, kRankFormPredict, row_bce_dev && row_kl_dev, cond_dev, eps_dev, 0, batch, targets));
    if (row0 < 0 || row0 > 0x7FFFFFFF - (int64_t)batch->n_rows) return fail(AAE_EINVAL, "aae_vae_predict_loss: row0 outside [0, 2^31 - n_rows)");
    return model_loss(m, rank_input(true, batch, cond_dev, eps_dev, nullptr, 0, (int)row0), targets, row_bce_dev, row_kl_dev, stream);
}

int aae_vae_decode_loss(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* targets,
                        double* row_bce_dev, void* stream) {
    TRY(loss_check_call("aae_vae_decode_loss", m, true, kRankFormDecode, zc_dev && row_bce_dev, nullptr, nullptr, zc_ld, batch, targets));
    return model_loss(m, rank_input(true, batch, nullptr, nullptr, zc_dev, zc_ld), targets, row_bce_dev, nullptr, stream);
}

int aae_loss_max_rows(aae_handle m, int32_t* rows_out) {
    TRY(rank_check_call("aae_loss_max_rows", m, false, kRankFormRows, rows_out, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
    *rows_out = loss_max_rows(m, false);
    return AAE_OK;
}

int aae_vae_loss_max_rows(aae_handle m, int32_t* rows_out) {
    TRY(rank_check_call("aae_vae_loss_max_rows", m, true, kRankFormRows, rows_out, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
    *rows_out = loss_max_rows(m, true);
    return AAE_OK;
}

int aae_rank_long_stats(aae_handle m, int64_t out[5]) {
    if (!m || !out) return fail(AAE_EINVAL, "NULL argument");
    for (int i = 0; i < 5; ++i) { out[i] = m->long_stats[i]; m->long_stats[i] = 0; }
    return AAE_OK;
}

// ---- the VAE: predict -> rank (reference vae.py:229-266 + evaluation.py:183-199, 20-58; abi_rank.h, the VAE's form) -------------------
int aae_vae_predict_topk(aae_handle m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, int32_t k,
                         int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    TRY(rank_check_call("aae_vae_predict_topk", m, true, kRankFormPredict, idx_out_dev && val_out_dev, &k, cond_dev, eps_dev, 0, batch, nullptr));
    return model_topk(m, rank_input(true, batch, cond_dev, eps_dev, nullptr, 0), k, exclude_known, idx_out_dev, val_out_dev, stream);
}

int aae_vae_decode_topk(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, int32_t k, int32_t exclude_known,
                        int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    TRY(rank_check_call("aae_vae_decode_topk", m, true, kRankFormDecode, zc_dev && idx_out_dev && val_out_dev, &k, nullptr, nullptr, zc_ld, batch, nullptr));
    return model_topk(m, rank_input(true, batch, nullptr, nullptr, zc_dev, zc_ld), k, exclude_known, idx_out_dev, val_out_dev, stream);
}

int aae_vae_predict_ranks(aae_handle m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, const aae_batch* truth,
                          int32_t exclude_known, int32_t* ranks_out_dev, void* stream) {
    TRY(rank_check_call("aae_vae_predict_ranks", m, true, kRankFormPredict, ranks_out_dev, nullptr, cond_dev, eps_dev, 0, batch, truth));
    return model_ranks(m, rank_input(true, batch, cond_dev, eps_dev, nullptr, 0), truth, exclude_known, ranks_out_dev, stream);
}

int aae_vae_decode_ranks(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* truth,
                         int32_t exclude_known, int32_t* ranks_out_dev, void* stream) {
    TRY(rank_check_call("aae_vae_decode_ranks", m, true, kRankFormDecode, zc_dev && ranks_out_dev, nullptr, nullptr, nullptr, zc_ld, batch, truth));
    return model_ranks(m, rank_input(true, batch, nullptr, nullptr, zc_dev, zc_ld), truth, exclude_known, ranks_out_dev, stream);
}

int aae_vae_rank_max_rows(aae_handle m, int32_t k, int32_t* rows_out) {
    TRY(rank_check_call("aae_vae_rank_max_rows", m, true, kRankFormRows, rows_out, &k, nullptr, nullptr, 0, nullptr, nullptr));
    *rows_out = std::max(m->R, rank_rows_cap(m, k, true));
    return AAE_OK;
}

int aae_vae_rank_full_max_rows(aae_handle m, int32_t* rows_out) {
    TRY(rank_check_call("aae_vae_rank_full_max_rows", m, true, kRankFormRows, rows_out, nullptr, nullptr, nullptr, 0, nullptr, nullptr));
    *rows_out = std::max(m->R, rank_full_rows_cap(m, true));
    return AAE_OK;
}

}  // extern "C"
