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

int aae_decode(aae_handle m, const float* zc_dev, int64_t zc_ld, int32_t n_rows, float* out_dev, int64_t out_ld,
               void* stream) {
    if (!m || !out_dev) return fail(AAE_EINVAL, "handle/out is NULL");
    if (n_rows < 1 || n_rows > m->R) return fail(AAE_EINVAL, "n_rows outside [1, max_batch]");
    if (out_ld < m->N || (out_ld & 3) || (reinterpret_cast<uintptr_t>(out_dev) & 15))
        return fail(AAE_EINVAL, "out_dev must be 16-byte aligned with out_ld >= n_items and out_ld % 4 == 0");
    hipStream_t s = S(stream);
    TRY(join_deferred(m, s));
    if (zc_dev) TRY(stage_zc(m, zc_dev, zc_ld, n_rows, s));
    if (m->vae) TRY(chain_vae_dec_hidden(m, n_rows, s));       // (VAE: one hidden layer, fc3)
    else if (m->use_chain) TRY(chain_dec_hidden(m, false, n_rows, s));
    else TRY(decoder_hidden_forward(m, false, nullptr, nullptr, n_rows, s));
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
    if (k <= 10)
        hipLaunchKernelGGL(topk_rows_kernel<10>, dim3(m->rows), dim3(256), 0, s, m->G.p, m->ldn, m->N, m->bv,
                           exclude_known, k, reinterpret_cast<int*>(idx_out_dev), val_out_dev);
    else if (k <= 20)
        hipLaunchKernelGGL(topk_rows_kernel<20>, dim3(m->rows), dim3(256), 0, s, m->G.p, m->ldn, m->N, m->bv,
                           exclude_known, k, reinterpret_cast<int*>(idx_out_dev), val_out_dev);
    else
        hipLaunchKernelGGL(topk_rows_kernel<32>, dim3(m->rows), dim3(256), 0, s, m->G.p, m->ldn, m->N, m->bv,
                           exclude_known, k, reinterpret_cast<int*>(idx_out_dev), val_out_dev);
    LAUNCHCHK("topk_rows");
    return AAE_OK;
}
// the dense form's scores: rows of `batch` (<= max_batch) into the [max_batch][n_items] scratch
int aae_scores_to_scratch(aae_model* m, const aae_batch* batch, const float* cond_dev, const float* zc_dev, int64_t zc_ld, void* stream) {
    if (!zc_dev) return aae_predict(m, batch, cond_dev, m->G.p, m->ldn, stream);
    TRY(set_batch(m, batch));
    return aae_decode(m, zc_dev, zc_ld, m->rows, m->G.p, m->ldn, stream);
}
// The four ranking calls of an AAE / AE handle.  zc_dev != NULL: the decode form - a caller-built decoder input (code |
// imposed conditions of any plugin kind), the second half of predict (aae.py:855-866); `batch` names the input rows whose
// items are excluded and cond_dev is not read.
int aae_topk(aae_model* m, const aae_batch* batch, const float* cond_dev, const float* zc_dev, int64_t zc_ld, int k, int exclude_known,
             int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    hipStream_t s = S(stream);
    if (batch->n_rows >= 1 && batch->n_rows <= rank_rows_cap(m, k)) {   // fused: no [rows][N] matrix (abi_rank.h)
        m->phase = 0;
        if (zc_dev) TRY(rank_decode(m, zc_dev, zc_ld, batch, k, exclude_known, idx_out_dev, val_out_dev, s));
        else TRY(rank_predict(m, batch, cond_dev, k, exclude_known, idx_out_dev, val_out_dev, s));
        if (!rank_long(k)) return AAE_OK;
        std::vector<std::pair<int, int>> spans;        // rows whose collect list overflowed: through the score matrix
        TRY(rank_long_overflow(m, batch, k, s, spans));
        for (const auto& sp : spans) {
            const aae_batch sub = rank_sub_batch(m, batch, sp.first, sp.second);
            const size_t r0 = (size_t)sp.first;
            TRY(aae_scores_to_scratch(m, &sub, cond_dev ? cond_dev + r0 * m->cfg.cond_inc : nullptr, zc_dev ? zc_dev + r0 * zc_ld : nullptr,
                                      zc_ld, stream));
            TRY(rank_long_dense(m, k, exclude_known, idx_out_dev + r0 * k, val_out_dev + r0 * k, s));
        }
        return AAE_OK;
    }
    TRY(aae_scores_to_scratch(m, batch, cond_dev, zc_dev, zc_ld, stream));
    TRY(topk_from_scores(m, k, exclude_known, idx_out_dev, val_out_dev, s));
    m->phase = 0;
    return AAE_OK;
}
// ... the rank of every held-out item in the full ranking of its row (rank_full.h)
int aae_ranks(aae_model* m, const aae_batch* batch, const float* cond_dev, const float* zc_dev, int64_t zc_ld, const aae_batch* truth,
              int exclude_known, int32_t* ranks_out_dev, void* stream) {
    hipStream_t s = S(stream);
    if (batch->n_rows >= 1 && batch->n_rows <= rank_full_rows_cap(m)) {     // fused: no [rows][N] matrix (abi_rank.h)
        m->phase = 0;
        if (zc_dev) return rank_full_decode(m, zc_dev, zc_ld, batch, truth, exclude_known, ranks_out_dev, s);
        return rank_full_predict(m, batch, cond_dev, truth, exclude_known, ranks_out_dev, s);
    }
    TRY(aae_scores_to_scratch(m, batch, cond_dev, zc_dev, zc_ld, stream));
    TRY(rank_full_dense(m, rank_view(batch), rank_view(truth), exclude_known, ranks_out_dev, s));
    m->phase = 0;
    return AAE_OK;
}
}  // namespace
extern "C" {

int aae_predict_topk(aae_handle m, const aae_batch* batch, const float* cond_dev, int32_t k, int32_t exclude_known,
                     int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    if (!m || !idx_out_dev || !val_out_dev) return fail(AAE_EINVAL, "NULL argument");
    TRY(rank_check_k("aae_predict_topk", k, m->N));
    if (m->cfg.cond_inc > 0 && !cond_dev) return fail(AAE_EINVAL, "cond_inc > 0 needs cond_dev");
    TRY(rank_check_batch(batch));
    return aae_topk(m, batch, cond_dev, nullptr, 0, k, exclude_known, idx_out_dev, val_out_dev, stream);
}

int aae_rank_max_rows(aae_handle m, int32_t k, int32_t* rows_out) {
    if (!m || !rows_out) return fail(AAE_EINVAL, "NULL argument");
    TRY(rank_check_k("aae_rank_max_rows", k, m->N));
    *rows_out = std::max(m->R, rank_rows_cap(m, k));
    return AAE_OK;
}

int aae_rank_long_stats(aae_handle m, int64_t out[5]) {
    if (!m || !out) return fail(AAE_EINVAL, "NULL argument");
    for (int i = 0; i < 5; ++i) { out[i] = m->long_stats[i]; m->long_stats[i] = 0; }
    return AAE_OK;
}

int aae_decode_topk(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, int32_t k,
                    int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    if (!m || !zc_dev || !idx_out_dev || !val_out_dev) return fail(AAE_EINVAL, "NULL argument");
    TRY(rank_check_k("aae_decode_topk", k, m->N));
    if (zc_ld < m->cp) return fail(AAE_EINVAL, "zc_ld < n_code + cond_inc");
    TRY(rank_check_batch(batch));
    return aae_topk(m, batch, nullptr, zc_dev, zc_ld, k, exclude_known, idx_out_dev, val_out_dev, stream);
}

int aae_rank_full_max_rows(aae_handle m, int32_t* rows_out) {
    if (!m || !rows_out) return fail(AAE_EINVAL, "NULL argument");
    *rows_out = std::max(m->R, rank_full_rows_cap(m));
    return AAE_OK;
}

int aae_predict_ranks(aae_handle m, const aae_batch* batch, const float* cond_dev, const aae_batch* truth, int32_t exclude_known,
                      int32_t* ranks_out_dev, void* stream) {
    if (!m || !ranks_out_dev) return fail(AAE_EINVAL, "NULL argument");
    if (m->cfg.cond_inc > 0 && !cond_dev) return fail(AAE_EINVAL, "cond_inc > 0 needs cond_dev");
    TRY(rank_check_batch(batch));
    TRY(rank_check_truth("aae_predict_ranks", batch->n_rows, truth));
    if (truth->max_row_nnz < 1) return fail(AAE_EINVAL, "aae_predict_ranks: truth needs max_row_nnz: the entries of its longest row (an upper bound)");
    return aae_ranks(m, batch, cond_dev, nullptr, 0, truth, exclude_known, ranks_out_dev, stream);
}

int aae_decode_ranks(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* truth,
                     int32_t exclude_known, int32_t* ranks_out_dev, void* stream) {
    if (!m || !zc_dev || !ranks_out_dev) return fail(AAE_EINVAL, "NULL argument");
    if (zc_ld < m->cp) return fail(AAE_EINVAL, "zc_ld < n_code + cond_inc");
    TRY(rank_check_batch(batch));
    TRY(rank_check_truth("aae_decode_ranks", batch->n_rows, truth));
    if (truth->max_row_nnz < 1) return fail(AAE_EINVAL, "aae_decode_ranks: truth needs max_row_nnz: the entries of its longest row (an upper bound)");
    return aae_ranks(m, batch, nullptr, zc_dev, zc_ld, truth, exclude_known, ranks_out_dev, stream);
}

}  // extern "C"

// ---- the VAE: predict -> rank (reference vae.py:229-266 + evaluation.py:183-199, 20-58; abi_rank.h, the VAE's form) -------------------
namespace {
int vae_rank_check(const aae_model* m, const float* cond_dev, const float* eps_dev, bool decode) {
    if (!m->vae || !m->use_chain) return fail(AAE_ESTATE, "model was not created in VAE mode (cfg.model_kind = 3)");
    if (decode) return AAE_OK;
    if (m->cfg.cond_inc > 0 && !cond_dev) return fail(AAE_EINVAL, "cond_inc > 0 needs cond_dev");
    if (m->cfg.rng_mode == AAE_RNG_INJECT && !eps_dev) return fail(AAE_EINVAL, "rng_mode inject needs eps_dev");
    return AAE_OK;
}
// the dense form's scores: rows of `batch` (<= max_batch) into the [max_batch][n_items] scratch
int vae_scores_to_scratch(aae_model* m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, const float* zc_dev,
                          int64_t zc_ld, void* stream) {
    if (!zc_dev) return aae_vae_predict(m, batch, cond_dev, eps_dev, m->G.p, m->ldn, stream);
    TRY(set_batch(m, batch));
    return aae_decode(m, zc_dev, zc_ld, m->rows, m->G.p, m->ldn, stream);
}
// zc_dev != NULL: the decode form (cond_dev / eps_dev are not read)
int vae_topk(aae_model* m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, const float* zc_dev, int64_t zc_ld,
             int k, int exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    hipStream_t s = S(stream);
    const int nc = m->c, ci = m->cfg.cond_inc;
    if (batch->n_rows >= 1 && batch->n_rows <= vae_rank_rows_cap(m, k)) {      // fused: no [rows][N] matrix
        const int rows = batch->n_rows;
        const VaeRankCopies c = vae_rank_copies(m, m->G.p);
        float* base = m->G.p + c.floats;
        const RankPlan p = rank_plan(m, rows, k, base);
        m->phase = 0;
        if (zc_dev) TRY(vae_rank_decode_hidden(m, zc_dev, zc_ld, rows, c, p.dh2, s));
        else TRY(vae_rank_predict_hidden(m, batch, cond_dev, eps_dev, 0, c, p.a1, p.eh1, p.rscale, p.dh2, s));
        TRY(rank_from_dh2(m, p, rank_view(batch), k, exclude_known, idx_out_dev, val_out_dev, s));
        if (!rank_long(k)) return AAE_OK;
        std::vector<std::pair<int, int>> spans;        // rows whose collect list overflowed: through the score matrix
        TRY(rank_long_overflow(m, batch, k, s, spans, base));
        for (const auto& sp : spans) {
            const aae_batch sub = rank_sub_batch(m, batch, sp.first, sp.second);
            const size_t r0 = (size_t)sp.first;
            TRY(vae_rank_long_span(m, &sub, cond_dev ? cond_dev + r0 * ci : nullptr, eps_dev ? eps_dev + r0 * nc : nullptr,
                                   zc_dev ? zc_dev + r0 * zc_ld : nullptr, zc_ld, sp.first, k, exclude_known, idx_out_dev + r0 * k,
                                   val_out_dev + r0 * k, s));
        }
        return AAE_OK;
    }
    TRY(vae_scores_to_scratch(m, batch, cond_dev, eps_dev, zc_dev, zc_ld, stream));
    TRY(topk_from_scores(m, k, exclude_known, idx_out_dev, val_out_dev, s));
    m->phase = 0;
    return AAE_OK;
}
int vae_ranks(aae_model* m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, const float* zc_dev, int64_t zc_ld,
              const aae_batch* truth, int exclude_known, int32_t* ranks_out_dev, void* stream) {
    hipStream_t s = S(stream);
    if (batch->n_rows >= 1 && batch->n_rows <= vae_rank_full_rows_cap(m)) {
        const int rows = batch->n_rows;
        const VaeRankCopies c = vae_rank_copies(m, m->G.p);
        const RankPlan p = rank_plan(m, rows, 32, m->G.p + c.floats, true);
        m->phase = 0;
        if (zc_dev) TRY(vae_rank_decode_hidden(m, zc_dev, zc_ld, rows, c, p.dh2, s));
        else TRY(vae_rank_predict_hidden(m, batch, cond_dev, eps_dev, 0, c, p.a1, p.eh1, p.rscale, p.dh2, s));
        return rank_full_from_dh2(m, p, rank_view(batch), rank_view(truth), truth->max_row_nnz, exclude_known, ranks_out_dev, s);
    }
    TRY(vae_scores_to_scratch(m, batch, cond_dev, eps_dev, zc_dev, zc_ld, stream));
    TRY(rank_full_dense(m, rank_view(batch), rank_view(truth), exclude_known, ranks_out_dev, s));
    m->phase = 0;
    return AAE_OK;
}
}  // namespace
extern "C" {

int aae_vae_predict_topk(aae_handle m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, int32_t k,
                         int32_t exclude_known, int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    if (!m || !idx_out_dev || !val_out_dev) return fail(AAE_EINVAL, "NULL argument");
    TRY(vae_rank_check(m, cond_dev, eps_dev, false));
    TRY(rank_check_k("aae_vae_predict_topk", k, m->N));
    TRY(rank_check_batch(batch));
    return vae_topk(m, batch, cond_dev, eps_dev, nullptr, 0, k, exclude_known, idx_out_dev, val_out_dev, stream);
}

int aae_vae_decode_topk(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, int32_t k, int32_t exclude_known,
                        int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    if (!m || !zc_dev || !idx_out_dev || !val_out_dev) return fail(AAE_EINVAL, "NULL argument");
    TRY(vae_rank_check(m, nullptr, nullptr, true));
    TRY(rank_check_k("aae_vae_decode_topk", k, m->N));
    if (zc_ld < m->cp) return fail(AAE_EINVAL, "zc_ld < n_code + cond_inc");
    TRY(rank_check_batch(batch));
    return vae_topk(m, batch, nullptr, nullptr, zc_dev, zc_ld, k, exclude_known, idx_out_dev, val_out_dev, stream);
}

int aae_vae_predict_ranks(aae_handle m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, const aae_batch* truth,
                          int32_t exclude_known, int32_t* ranks_out_dev, void* stream) {
    if (!m || !ranks_out_dev) return fail(AAE_EINVAL, "NULL argument");
    TRY(vae_rank_check(m, cond_dev, eps_dev, false));
    TRY(rank_check_batch(batch));
    TRY(rank_check_truth("aae_vae_predict_ranks", batch->n_rows, truth));
    if (truth->max_row_nnz < 1) return fail(AAE_EINVAL, "aae_vae_predict_ranks: truth needs max_row_nnz: the entries of its longest row (an upper bound)");
    return vae_ranks(m, batch, cond_dev, eps_dev, nullptr, 0, truth, exclude_known, ranks_out_dev, stream);
}

int aae_vae_decode_ranks(aae_handle m, const float* zc_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* truth,
                         int32_t exclude_known, int32_t* ranks_out_dev, void* stream) {
    if (!m || !zc_dev || !ranks_out_dev) return fail(AAE_EINVAL, "NULL argument");
    TRY(vae_rank_check(m, nullptr, nullptr, true));
    if (zc_ld < m->cp) return fail(AAE_EINVAL, "zc_ld < n_code + cond_inc");
    TRY(rank_check_batch(batch));
    TRY(rank_check_truth("aae_vae_decode_ranks", batch->n_rows, truth));
    if (truth->max_row_nnz < 1) return fail(AAE_EINVAL, "aae_vae_decode_ranks: truth needs max_row_nnz: the entries of its longest row (an upper bound)");
    return vae_ranks(m, batch, nullptr, nullptr, zc_dev, zc_ld, truth, exclude_known, ranks_out_dev, stream);
}

int aae_vae_rank_max_rows(aae_handle m, int32_t k, int32_t* rows_out) {
    if (!m || !rows_out) return fail(AAE_EINVAL, "NULL argument");
    TRY(vae_rank_check(m, nullptr, nullptr, true));
    TRY(rank_check_k("aae_vae_rank_max_rows", k, m->N));
    *rows_out = std::max(m->R, vae_rank_rows_cap(m, k));
    return AAE_OK;
}

int aae_vae_rank_full_max_rows(aae_handle m, int32_t* rows_out) {
    if (!m || !rows_out) return fail(AAE_EINVAL, "NULL argument");
    TRY(vae_rank_check(m, nullptr, nullptr, true));
    *rows_out = std::max(m->R, vae_rank_full_rows_cap(m));
    return AAE_OK;
}

}  // extern "C"
