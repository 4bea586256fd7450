// Entry points of IRGAN (irgan.h): scores alone, scores into the caller's scratch followed by the dense ranking calls of
// abi_rank.h as they stand, and the three training calls, each of which loops over its steps HERE - the host is not entered per
// step.  Handle-free like the lowrank / rand calls: every buffer is the caller's, every launch goes to the caller's stream,
// nothing synchronises.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

static_assert(kIrDimMax == AAE_IRGAN_DIM_MAX && kIrPosMax == AAE_IRGAN_POS_MAX && kIrBatchMax == AAE_IRGAN_BATCH_MAX &&
              kIrTile == AAE_IRGAN_TILE, "include/aaerec_hip.h names the limits of csrc/irgan.h");

namespace {

// the caller's scratch: a fixed region, then one table slot per user a launch works on at once
struct IrLayout {
    int tiles, utiles;
    size_t hdr, part, l2, smp, coef, tu, ti, g, bce, ru, rv, slots, slot, need;
};
IrLayout ir_layout(const aae_irgan_net* n) {
    IrLayout L;
    L.tiles = (n->items + kIrTile - 1) / kIrTile; L.utiles = (n->users + kIrTile - 1) / kIrTile;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
    L.hdr = take(8 * sizeof(double));
    L.part = take((size_t)L.tiles * n->dim * sizeof(double));
    L.l2 = take((size_t)(L.utiles + 2 * L.tiles) * sizeof(double));
    L.smp = take(2 * kIrPosMax * sizeof(int32_t)); L.coef = take(2 * kIrPosMax * sizeof(float));
    L.tu = take(2 * kIrBatchMax * sizeof(int32_t)); L.ti = take(2 * kIrBatchMax * sizeof(int32_t));
    L.g = take(2 * kIrBatchMax * sizeof(float)); L.bce = take(2 * kIrBatchMax * sizeof(float));
    L.ru = take((size_t)2 * kIrBatchMax * n->dim * sizeof(float)); L.rv = take((size_t)2 * kIrBatchMax * n->dim * sizeof(float));
    L.slots = o;
    L.slot = (size_t)L.tiles * (3 * sizeof(double) + kIrTile * sizeof(float));
    L.need = L.slots + L.slot;
    return L;
}

int ir_check_net(const std::string& w, const aae_irgan_net* n, const char* name, bool momentum) {
    if (!n || !n->user_emb_dev || !n->item_emb_dev || !n->item_bias_dev) return fail(AAE_EINVAL, w + ": " + name + " or one of its parameters is NULL");
    if (momentum && (!n->m_user_emb_dev || !n->m_item_emb_dev || !n->m_item_bias_dev))
        return fail(AAE_EINVAL, w + ": a momentum buffer of " + name + " is NULL");
    if (n->dim < 1 || n->dim > kIrDimMax) return fail(AAE_EINVAL, w + ": " + name + "->dim must be in [1, 64]");
    if (n->users < 1 || n->items < 1) return fail(AAE_EINVAL, w + ": " + name + "->users and ->items must be positive");
    return AAE_OK;
}
int ir_check_scratch(const std::string& w, const aae_irgan_net* n, const void* scratch, size_t bytes) {
    if (!scratch) return fail(AAE_EINVAL, w + ": the scratch is NULL");
    if (reinterpret_cast<uintptr_t>(scratch) & 255) return fail(AAE_EINVAL, w + ": the scratch must be 256-byte aligned");
    if (bytes < ir_layout(n).need) return fail(AAE_EINVAL, w + ": the scratch is smaller than aae_irgan_scratch_bytes()");
    return AAE_OK;
}
IrNet ir_net(const aae_irgan_net* n) {
    return IrNet{n->user_emb_dev, n->item_emb_dev, n->item_bias_dev, n->m_user_emb_dev, n->m_item_emb_dev, n->m_item_bias_dev,
                 n->users, n->items, n->dim};
}

int irgan_score_check(const char* who, const aae_irgan_net* g, const int32_t* users_dev, int32_t n_rows, const int64_t* pos_indptr_dev,
                      const int32_t* pos_items_dev, const float* out, int64_t ld) {
    const std::string w(who);
    TRY(ir_check_net(w, g, "gen", false));
    if (!users_dev) return fail(AAE_EINVAL, w + ": users_dev is NULL");
    if (n_rows < 0) return fail(AAE_EINVAL, w + ": the row count is negative");
    if ((pos_indptr_dev == nullptr) != (pos_items_dev == nullptr))
        return fail(AAE_EINVAL, w + ": pos_indptr_dev and pos_items_dev are one CSR: both or neither");
    if (!out) return fail(AAE_EINVAL, w + ": the score matrix (scratch) is NULL");
    if (ld < g->items) return fail(AAE_EINVAL, w + ": the score matrix's leading dimension (ld) is smaller than gen->items");
    if ((ld & 3) || ld > 0x7FFFFFFF || !aligned16(out))
        return fail(AAE_EINVAL, w + ": the score matrix's leading dimension must be a multiple of 4 floats below 2^31 on a 16-byte aligned base");
    return AAE_OK;
}
int irgan_score_launch(const aae_irgan_net* g, const int32_t* users_dev, int32_t n_rows, const int64_t* pos_indptr_dev,
                       const int32_t* pos_items_dev, float* out, int64_t ld, hipStream_t s) {
    const int tiles = (g->items + kIrTile - 1) / kIrTile;
    hipLaunchKernelGGL(irgan_scores_kernel, dim3((unsigned)tiles, (unsigned)std::min(n_rows, 1024)), dim3(kIrTile), 0, s, ir_net(g), users_dev,
                       n_rows, pos_indptr_dev, pos_items_dev, out, (long long)ld);
    LAUNCHCHK("irgan_scores");
    return AAE_OK;
}

}  // namespace

extern "C" {

int aae_irgan_scratch_bytes(const aae_irgan_net* net, size_t* bytes_out) {
    TRY(ir_check_net("aae_irgan_scratch_bytes", net, "net", false));
    if (!bytes_out) return fail(AAE_EINVAL, "aae_irgan_scratch_bytes: bytes_out is NULL");
    *bytes_out = ir_layout(net).need;
    return AAE_OK;
}

int aae_irgan_scores(const aae_irgan_net* gen, const int32_t* users_dev, int32_t n_rows, const int64_t* pos_indptr_dev,
                     const int32_t* pos_items_dev, float* out_dev, int64_t ld, void* stream) {
    TRY(irgan_score_check("aae_irgan_scores", gen, users_dev, n_rows, pos_indptr_dev, pos_items_dev, out_dev, ld));
    if (n_rows == 0) return AAE_OK;
    return irgan_score_launch(gen, users_dev, n_rows, pos_indptr_dev, pos_items_dev, out_dev, ld, S(stream));
}

int aae_irgan_topk(const aae_irgan_net* gen, const int32_t* users_dev, const int64_t* pos_indptr_dev, const int32_t* pos_items_dev,
                   const aae_batch* known, int32_t k, int32_t exclude_known, float* scratch_dev, int64_t scratch_ld,
                   int32_t* idx_out_dev, float* val_out_dev, void* stream) {
    const char* who = "aae_irgan_topk";
    if (!known || !known->indptr_dev || !known->indices_dev) return fail(AAE_EINVAL, std::string(who) + ": the known-item batch pointers are NULL");
    TRY(irgan_score_check(who, gen, users_dev, known->n_rows, pos_indptr_dev, pos_items_dev, scratch_dev, scratch_ld));
    TRY(rank_check_k(who, k, gen->items));
    TRY(rank_check_lists(who, idx_out_dev, val_out_dev));
    if (known->n_rows == 0) return AAE_OK;
    TRY(irgan_score_launch(gen, users_dev, known->n_rows, pos_indptr_dev, pos_items_dev, scratch_dev, scratch_ld, S(stream)));
    return dense_topk(scratch_dev, scratch_ld, gen->items, rank_view(known), known->n_rows, k, exclude_known, idx_out_dev, val_out_dev, S(stream));
}

int aae_irgan_ranks(const aae_irgan_net* gen, const int32_t* users_dev, const int64_t* pos_indptr_dev, const int32_t* pos_items_dev,
                    const aae_batch* known, const aae_batch* truth, int32_t exclude_known, float* scratch_dev, int64_t scratch_ld,
                    int32_t* ranks_out_dev, void* stream) {
    const char* who = "aae_irgan_ranks";
    if (!known || !known->indptr_dev || !known->indices_dev) return fail(AAE_EINVAL, std::string(who) + ": the known-item batch pointers are NULL");
    TRY(irgan_score_check(who, gen, users_dev, known->n_rows, pos_indptr_dev, pos_items_dev, scratch_dev, scratch_ld));
    TRY(rank_check_truth(who, known->n_rows, truth));
    if (!ranks_out_dev) return fail(AAE_EINVAL, std::string(who) + ": ranks_out_dev is NULL");
    if (known->n_rows == 0) return AAE_OK;
    TRY(irgan_score_launch(gen, users_dev, known->n_rows, pos_indptr_dev, pos_items_dev, scratch_dev, scratch_ld, S(stream)));
    return dense_ranks(scratch_dev, scratch_ld, gen->items, rank_view(known), rank_view(truth), known->n_rows, exclude_known, ranks_out_dev,
                       S(stream));
}

int aae_irgan_d_steps(const aae_irgan_net* dis, const int32_t* lines_dev, int64_t n_lines, int32_t batch_size, int32_t n_steps, float lr,
                      float momentum, float lambda, double* losses_out_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    const std::string w("aae_irgan_d_steps");
    TRY(ir_check_net(w, dis, "dis", true));
    if (!lines_dev) return fail(AAE_EINVAL, w + ": lines_dev is NULL");
    if (batch_size < 1 || batch_size > kIrBatchMax) return fail(AAE_EINVAL, w + ": batch_size must be in [1, 1024] lines");
    if (n_lines < 0 || n_steps < 0 || (int64_t)n_steps > (n_lines + batch_size - 1) / batch_size)
        return fail(AAE_EINVAL, w + ": n_steps must be in [0, ceil(n_lines / batch_size)]");
    TRY(ir_check_scratch(w, dis, scratch_dev, scratch_bytes));
    const IrLayout L = ir_layout(dis);
    char* base = static_cast<char*>(scratch_dev);
    auto at = [&](size_t off) { return base + off; };
    IrDScratch W;
    W.tu = reinterpret_cast<int32_t*>(at(L.tu)); W.ti = reinterpret_cast<int32_t*>(at(L.ti));
    W.g = reinterpret_cast<float*>(at(L.g)); W.bce = reinterpret_cast<float*>(at(L.bce));
    W.ru = reinterpret_cast<float*>(at(L.ru)); W.rv = reinterpret_cast<float*>(at(L.rv));
    W.l2 = reinterpret_cast<double*>(at(L.l2));
    const IrNet D = ir_net(dis);
    hipStream_t s = S(stream);
    // the gradient of lambda * mean(p^2): 2 lambda p / size
    const float reg_u = (float)(2.0 * lambda / ((double)dis->users * dis->dim)), reg_v = (float)(2.0 * lambda / ((double)dis->items * dis->dim)),
                reg_b = (float)(2.0 * lambda / (double)dis->items);
    for (int st = 0; st < n_steps; ++st) {
        const int64_t first = (int64_t)st * batch_size;
        const int nl = (int)std::min<int64_t>(batch_size, n_lines - first);
        hipLaunchKernelGGL(irgan_d_prep_kernel, dim3((unsigned)((2 * nl + kIrTile - 1) / kIrTile)), dim3(kIrTile), 0, s, D, lines_dev + 3 * first,
                           nl, W);
        LAUNCHCHK("irgan_d_prep");
        hipLaunchKernelGGL(irgan_d_update_kernel, dim3((unsigned)(L.utiles + L.tiles)), dim3(kIrTile), 0, s, D, 2 * nl, W, L.utiles, L.tiles, lr,
                           momentum, reg_u, reg_v, reg_b);
        LAUNCHCHK("irgan_d_update");
        if (losses_out_dev) {
            hipLaunchKernelGGL(irgan_d_loss_kernel, dim3(1), dim3(kIrTile), 0, s, D, 2 * nl, W, L.utiles, L.tiles, (double)lambda,
                               losses_out_dev + st);
            LAUNCHCHK("irgan_d_loss");
        }
    }
    return AAE_OK;
}

int aae_irgan_sample_neg(const aae_irgan_net* gen, const int32_t* users_dev, const int64_t* line_off_dev, int32_t n_users, int32_t max_pos,
                         float temperature, uint64_t seed, int64_t draw, int32_t* lines_dev, int64_t n_lines, void* scratch_dev,
                         size_t scratch_bytes, void* stream) {
    const std::string w("aae_irgan_sample_neg");
    TRY(ir_check_net(w, gen, "gen", false));
    if (!users_dev || !line_off_dev || !lines_dev) return fail(AAE_EINVAL, w + ": users_dev / line_off_dev / lines_dev is NULL");
    if (n_users < 0 || n_lines < 0 || draw < 0) return fail(AAE_EINVAL, w + ": a negative count or draw");
    if (max_pos < 0 || max_pos > kIrPosMax) return fail(AAE_EINVAL, w + ": a user with more than 2048 positives (max_pos)");
    if (!(temperature > 0.f)) return fail(AAE_EINVAL, w + ": the temperature must be positive");
    TRY(ir_check_scratch(w, gen, scratch_dev, scratch_bytes));
    const IrLayout L = ir_layout(gen);
    char* slots = static_cast<char*>(scratch_dev) + L.slots;
    const int per = (int)std::min<size_t>((scratch_bytes - L.slots) / L.slot, 4096);
    const IrNet G = ir_net(gen);
    hipStream_t s = S(stream);
    for (int q0 = 0; q0 < n_users; q0 += per) {
        const int q = std::min(per, n_users - q0);
        hipLaunchKernelGGL(irgan_logits_kernel, dim3((unsigned)L.tiles, (unsigned)q), dim3(kIrTile), 0, s, G, users_dev, q0, 1.f / temperature, slots,
                           L.slot);
        LAUNCHCHK("irgan_logits");
        hipLaunchKernelGGL(irgan_draw_neg_kernel, dim3((unsigned)q), dim3(kIrTile), 0, s, G, users_dev, line_off_dev, q0, L.tiles, seed,
                           (uint64_t)draw, n_lines, lines_dev, slots, L.slot);
        LAUNCHCHK("irgan_draw_neg");
    }
    return AAE_OK;
}

int aae_irgan_g_steps(const aae_irgan_net* gen, const aae_irgan_net* dis, const int32_t* users_dev, int32_t n_steps,
                      const int64_t* pos_indptr_dev, const int32_t* pos_items_dev, int32_t max_pos, const int32_t* samples_dev,
                      const int64_t* sample_off_dev, int32_t* samples_out_dev, uint64_t seed, int64_t draw, float lr, float momentum,
                      double* losses_out_dev, void* scratch_dev, size_t scratch_bytes, void* stream) {
    const std::string w("aae_irgan_g_steps");
    TRY(ir_check_net(w, gen, "gen", true));
    TRY(ir_check_net(w, dis, "dis", false));
    if (gen->users != dis->users || gen->items != dis->items) return fail(AAE_EINVAL, w + ": gen and dis name other numbers of users or items");
    if (!users_dev || !pos_indptr_dev || !pos_items_dev) return fail(AAE_EINVAL, w + ": users_dev / pos_indptr_dev / pos_items_dev is NULL");
    if ((samples_dev != nullptr || samples_out_dev != nullptr) != (sample_off_dev != nullptr))
        return fail(AAE_EINVAL, w + ": sample_off_dev comes with samples_dev or samples_out_dev: both or neither");
    if (n_steps < 0 || draw < 0) return fail(AAE_EINVAL, w + ": a negative count or draw");
    if (max_pos < 0 || max_pos > kIrPosMax) return fail(AAE_EINVAL, w + ": a user with more than 2048 positives (max_pos)");
    TRY(ir_check_scratch(w, gen, scratch_dev, scratch_bytes));
    const IrLayout L = ir_layout(gen);
    char* base = static_cast<char*>(scratch_dev);
    char* slots = base + L.slots;
    const IrNet G = ir_net(gen), D = ir_net(dis);
    hipStream_t s = S(stream);
    IrGStep A;
    A.users = users_dev; A.pos_indptr = pos_indptr_dev; A.pos_items = pos_items_dev; A.samples = samples_dev; A.sample_off = sample_off_dev; A.smp_out = samples_out_dev;
    A.seed = seed; A.draw = (uint64_t)draw;
    A.hdr = reinterpret_cast<double*>(base + L.hdr); A.smp = reinterpret_cast<int32_t*>(base + L.smp); A.coef = reinterpret_cast<float*>(base + L.coef);
    double* part = reinterpret_cast<double*>(base + L.part);
    for (int st = 0; st < n_steps; ++st) {
        A.step = st; A.loss_out = losses_out_dev ? losses_out_dev + st : nullptr;
        hipLaunchKernelGGL(irgan_logits_kernel, dim3((unsigned)L.tiles, 1), dim3(kIrTile), 0, s, G, users_dev, st, 1.f, slots, (size_t)0);
        LAUNCHCHK("irgan_logits");
        hipLaunchKernelGGL(irgan_g_sample_kernel, dim3(1), dim3(kIrTile), 0, s, G, D, A, L.tiles, slots);
        LAUNCHCHK("irgan_g_sample");
        hipLaunchKernelGGL(irgan_g_update_kernel, dim3((unsigned)(L.tiles + L.utiles)), dim3(kIrTile), 0, s, G, A, L.tiles, slots, part, lr, momentum);
        LAUNCHCHK("irgan_g_update");
        hipLaunchKernelGGL(irgan_g_user_kernel, dim3(1), dim3(kIrUserParts * kIrDimMax), 0, s, G, A, L.tiles, part, lr, momentum);
        LAUNCHCHK("irgan_g_user");
    }
    return AAE_OK;
}

}  // extern "C"
