// predict -> rank fused (rank_x3.h): the host side behind aae_predict_topk / aae_decode_topk / aae_rank_max_rows.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
//
// One call ranks up to aae_rank_max_rows() rows - more than the training batch: nothing of it uses the handle's per-batch
// buffers.  Its workspace is the arena's [max_batch][n_items] scratch (AAE_T_ACT_G: the training step's dL/dlogits tiles,
// free between steps once the deferred optimiser launch is joined) + the dA2 slab area behind it:
//   a1 / eh1 [rows][ldh]    first-layer pre-activations / activations (enc_gather_kernel)
//   dh2      [rows][ldh]    the decoder's last hidden activations (ONE chain program: encoder tail -> code -> condition
//                           block -> decoder hidden layers, 4 rows per workgroup)
//   known    [rows][kw]     bitmap of the rows' input items        cand [rows][wgs][K] x (score, id), mm [rows][wgs][2]
//   k > 32 (rank_long.h):   tau [rows], count [rows], list [rows][cap] x 64 bits
// Launches per call: (deferred-Adam flush of enc.lin1 when rows are behind) gather, chain, known-item mask, rank, merge.
// k > 32: ... rank (K = 32), floor, rank again with the collect epilogue, sort; then the rows' counts are read back (the call
// synchronises its stream) and a row whose list overflowed is ranked through the score matrix (rank_long_dense).
// Full ranking (rank_full.h; aae_predict_ranks / aae_decode_ranks): no candidate lists; instead
//   tgt_i, tgt_v, tcount [rows][kFullSlots]   the held-out items of this round, their logits, the cells ranked before them
// Launches: gather, chain, known-item mask, then per round of 8 held-out items a row: setup, rank (pick), rank (count), finish.
// Held-out loss (loss_eval.h; aae_predict_loss / aae_decode_loss / aae_vae_*): no lists, no target slots; instead
//   lpart [rows][wgs] doubles, csum [rows][kLossChunksMax] doubles, (VAE) mulv [rows][2 n_code]
// Launches: gather, chain, TARGET mask, rank (loss), loss_targets, loss_finish, (VAE, predict form) vae_kl_rows.
// One host path for both kinds of handle and both forms of a call (the drivers model_topk / model_ranks, abi_predict.h):
//   RankInput + rank_cut    the rows of a call - batch, cond, eps, zc, generator row - and a span of them: the only place that
//                           knows their strides
//   rank_ws, rank_cap       the workspace's one layout (a VAE handle's weight copies in front of the plan) and its row limits
//   rank_hidden             the hidden half: the program builder of this handle and form -> p.dh2
//   rank_from_dh2 / rank_full_from_dh2      p.dh2 -> lists / ranks
//   loss_from_dh2                           p.dh2 -> the rows' BCE sums against a target CSR (loss_eval.h; model_loss)
//   rank_check_call         the argument check of the eight entry points and the four *_max_rows
#pragma once

namespace {

constexpr int kRankMaxRows = 4096;

struct RankPlan {
    int rows, K, nblk, wgs, kw, bb;
    float *a1, *eh1, *dh2, *rscale, *cand_v, *mm; int* cand_i; unsigned* known;
    int cap; float* tau; int* count; unsigned long long* list;      // k > 32 (rank_long.h)
    int* tgt_i; float* tgt_v; int* tcount;                          // full ranking (rank_full.h)
    double *lpart, *csum; float* mulv;                              // held-out loss (loss_eval.h); mulv: a VAE handle's [mu | logvar]
    size_t floats;
};

// what a plan lays out behind the hidden half and the mask: candidate lists, the full ranking's slots, the loss's sums
enum { kPlanLists = 0, kPlanFull = 1, kPlanLoss = 2 };

inline bool rank_long(int k) { return k > 32; }
inline int rank_collect_cap(const aae_model* m) { return m->opt.rank_collect_cap > 0 ? m->opt.rank_collect_cap : kLongCap; }

inline int rank_K(int k) { return k <= 10 ? 10 : k <= 20 ? 20 : 32; }

// lays the workspace out for `rows` rows (base == NULL: measures only)
RankPlan rank_plan(const aae_model* m, int rows, int k, float* base, int layout = kPlanLists) {
    RankPlan p; memset(&p, 0, sizeof(p));
    p.rows = rows; p.K = rank_K(k);
    const int ntiles = (m->N + kTI - 1) / kTI;
    p.bb = kRankGR2;          // (both rank kernels: 128-row blocks, rank_x3.h)
    p.nblk = (rows + p.bb - 1) / p.bb;
    p.wgs = std::max(1, std::min(m->n_cu / std::max(1, p.nblk), ntiles));
    p.kw = (m->N + 31) / 32;
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n + 63) & ~(size_t)63; return base ? base + o : nullptr; };
    p.a1 = take((size_t)rows * m->ldh); p.eh1 = take((size_t)rows * m->ldh); p.dh2 = take((size_t)rows * m->ldh);
    p.rscale = take(rows);
    p.known = reinterpret_cast<unsigned*>(take((size_t)rows * p.kw));
    if (layout == kPlanLoss) {     // (no lists, no slots: doubles - every offset is a multiple of 64 floats)
        p.lpart = reinterpret_cast<double*>(take((size_t)rows * p.wgs * 2));
        p.csum = reinterpret_cast<double*>(take((size_t)rows * kLossChunksMax * 2));
        if (m->vae) p.mulv = take((size_t)rows * 2 * m->c);
        p.floats = off;
        return p;
    }
    if (layout == kPlanFull) {     // (no lists: the pick / count epilogues leave no candidates)
        p.tgt_i = reinterpret_cast<int*>(take((size_t)rows * kFullSlots));
        p.tgt_v = take((size_t)rows * kFullSlots);
        p.tcount = reinterpret_cast<int*>(take((size_t)rows * kFullSlots));
        p.floats = off;
        return p;
    }
    p.cand_v = take((size_t)rows * p.wgs * p.K);
    p.cand_i = reinterpret_cast<int*>(take((size_t)rows * p.wgs * p.K));
    p.mm = take((size_t)rows * p.wgs * 2);
    if (rank_long(k)) {
        p.cap = rank_collect_cap(m);
        p.tau = take(rows); p.count = reinterpret_cast<int*>(take(rows));
        p.list = reinterpret_cast<unsigned long long*>(take((size_t)rows * p.cap * 2));
    }
    p.floats = off;
    return p;
}

// the workspace: the [max_batch][n_items] scratch and, where the layout put them right behind it (it does), the dA2 slabs of
// the output layer - both hold data of a running step only, and a rank call runs between steps behind join_deferred()
size_t rank_ws_floats(const aae_model* m) {
    if (m->slabs.p && m->slabs.p > m->G.p) return (size_t)(m->slabs.p - m->G.p) + m->slabs.floats();
    return m->G.floats();
}

// A VAE handle keeps no k-major copies of its layers (its training programs run on chain.h, whose optimiser epilogues would
// have to keep them in step): a rank call derives the F4 copies of the two small matrices into the head of its workspace -
// ~60 k floats at the headline widths, two launches - and lays its plan out behind them.  An AAE / AE handle has no head.
struct VaeRankCopies { float* w3; float* v1; float* d4; size_t floats; };

VaeRankCopies vae_rank_copies(const aae_model* m, float* base) {
    VaeRankCopies c; memset(&c, 0, sizeof(c));
    if (!m->vae) return c;
    auto f4 = [](const Ten& W) { return (size_t)((W.cols + 3) / 4 + kW4Pad) * 4 * W.rows; };          // (+ the zero k-chunk rows, chain4.h)
    auto d4 = [](const Ten& W) { return (size_t)((W.rows + 3) / 4) * 4 * W.cols; };
    const Ten &W3 = m->P[P_W3], &V1 = m->P[P_V1];
    size_t off = 0;
    auto take = [&](size_t n) { size_t o = off; off += (n + 63) & ~(size_t)63; return base ? base + o : nullptr; };
    c.w3 = take(f4(W3)); c.v1 = take(f4(V1));
    c.d4 = take(std::max(d4(W3), d4(V1)));       // (interleave4_kernel writes the dX copy too: nobody reads it)
    c.floats = off;
    return c;
}

// a fused call's workspace, the only layout of it: the head, the plan behind it
struct RankWs { VaeRankCopies c; RankPlan p; };
RankWs rank_ws(const aae_model* m, int rows, int k, int layout) {
    RankWs w;
    w.c = vae_rank_copies(m, m->G.p);
    w.p = rank_plan(m, rows, k, m->G.p + w.c.floats, layout);
    return w;
}

// most rows one fused call (layout: kPlanFull - one fused full-ranking call - and kPlanLoss - one fused loss call - ask with
// k = 32) can take in `have` floats behind the head
int rank_rows_fit(const aae_model* m, int k, int layout, size_t have) {
    if (k < 1 || k > kLongKMax) return 0;
    const int ntiles = (m->N + kTI - 1) / kTI;
    int lo = 0, hi = kRankMaxRows;          // (the plan's size is monotone in rows up to rounding: bisect)
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        const RankPlan p = rank_plan(m, mid, k, nullptr, layout);
        // (k > 32: the floor needs k candidates per row - fewer workgroups per row block than that and every row would overflow)
        const bool floor_ok = !rank_long(k) || p.wgs * 32 >= k || p.wgs == ntiles;
        if (p.floats <= have && floor_ok) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// vae: the aae_vae_* family asks - a VAE handle ranks fused through those calls alone, any other handle through the aae_* ones
// (0: the fused path does not apply)
int rank_cap(const aae_model* m, int k, int layout, bool vae) {
    const size_t have = rank_ws_floats(m), head = vae_rank_copies(m, nullptr).floats;
    return (vae ? m->vae_rank_ok : m->rank_ok) && have > head ? rank_rows_fit(m, k, layout, have - head) : 0;
}
int rank_rows_cap(const aae_model* m, int k, bool vae) { return rank_cap(m, k, kPlanLists, vae); }
int rank_full_rows_cap(const aae_model* m, bool vae) { return rank_cap(m, 32, kPlanFull, vae); }
int rank_loss_rows_cap(const aae_model* m, bool vae) { return rank_cap(m, 32, kPlanLoss, vae); }

// one launch of a rank kernel: the lists' kernel of this (NB, K) (kernel_pick.h), or the K = 32 kernel's front end with
// another epilogue: collect (rank_long.h), pick / count (rank_full.h), loss (loss_eval.h)
int launch_rank(const RankArgs& a, int nb, int K, int epi, int grid, hipStream_t s) {
    const bool win = x3_big_span(a.N, a.ldv);      // (dec.lin3 beyond 2^31 bytes: the moving-window instantiations, dec_fused.h)
    const RankPick r = epi == kRankLists ? pick_rank_lists(nb, K, win) : pick_rank_epilogue(nb, epi, win);
    if (!r.kernel) return fail(AAE_ESTATE, "no rank kernel is compiled for this hidden width and list size");
    hipLaunchKernelGGL(r.kernel, dim3(grid), dim3(kNT), (uint32_t)r.lds, s, a);
    LAUNCHCHK(r.name);
    return AAE_OK;
}

// the known-item mask of the plan's rows, and what every rank launch over them is given (the pointers a plan does not lay
// out are NULL)
int rank_mask_and_args(aae_model* m, const RankPlan& p, const BatchView& bv, int exclude_known, RankArgs& a, hipStream_t s) {
    hipLaunchKernelGGL(known_mask_kernel, dim3(p.rows), dim3(256), 0, s, bv, exclude_known ? p.known : (unsigned*)nullptr, p.kw,
                       p.dh2, m->ldh, m->h);
    LAUNCHCHK("known_mask");
    memset(&a, 0, sizeof(a));
    a.dh2 = p.dh2; a.ldh = m->ldh; a.V3a = m->P[P_V3].p; a.ldv = m->ldh; a.N = m->N; a.B = p.rows;
    a.nblk = p.nblk; a.Bb = p.bb; a.known = exclude_known ? p.known : nullptr; a.kw = p.kw;
    a.cand_v = p.cand_v; a.cand_i = p.cand_i; a.mm = p.mm; a.one_term = m->bf16 ? 1 : 0;
    a.tgt_i = p.tgt_i; a.tgt_v = p.tgt_v; a.tcount = p.tcount; a.lpart = p.lpart;
    return AAE_OK;
}

// dh2 (workspace) of `rows` rows -> [rows][k] ids and scaled scores
int rank_from_dh2(aae_model* m, const RankPlan& p, const BatchView& bv, int k, int exclude_known, int32_t* idx_out,
                  float* val_out, hipStream_t s) {
    RankArgs a;
    TRY(rank_mask_and_args(m, p, bv, exclude_known, a, s));
    a.dbg = m->opt.rank_skip;
    const int grid = p.wgs * p.nblk;
    {
        ProfScope ps(m, AAE_K_RANK, s);
        TRY(launch_rank(a, m->fused_nb, p.K, kRankLists, grid, s));
    }
    if (rank_long(k)) {
        ProfScope ps(m, AAE_K_RANK, s);
        hipLaunchKernelGGL(rank_floor_kernel, dim3(p.rows), dim3(256), 0, s, p.cand_v, p.cand_i, p.wgs * p.K, k, p.tau, p.count);
        LAUNCHCHK("rank_floor");
        a.tau = p.tau; a.count = p.count; a.list = p.list; a.cap = p.cap;
        TRY(launch_rank(a, m->fused_nb, p.K, kRankCollect, grid, s));
        int P = 2;
        while (P < p.cap) P <<= 1;
        hipLaunchKernelGGL(rank_long_sort_kernel, dim3(p.rows), dim3(kLongNT), (uint32_t)(P * sizeof(unsigned long long)), s,
                           p.list, p.count, p.cap, p.mm, p.wgs, k, reinterpret_cast<int*>(idx_out), val_out);
        LAUNCHCHK("rank_long_sort");
        return AAE_OK;
    }
    const MergeKernel merge = pick_rank_merge(p.K);
    if (!merge) return fail(AAE_ESTATE, "no rank_merge kernel is compiled for this list size");
    hipLaunchKernelGGL(merge, dim3((p.rows + 3) / 4), dim3(256), 0, s, p.cand_v, p.cand_i, p.mm, p.rows, p.wgs, k,
                       reinterpret_cast<int*>(idx_out), val_out);
    LAUNCHCHK("rank_merge");
    return AAE_OK;
}

// dh2 (workspace) of `rows` rows -> the rank of every stored entry of the rows' truth, CSR order (rank_full.h)
int rank_full_from_dh2(aae_model* m, const RankPlan& p, const BatchView& bv, const BatchView& tv, int max_truth, int exclude_known,
                       int32_t* ranks_out, hipStream_t s) {
    RankArgs a;
    TRY(rank_mask_and_args(m, p, bv, exclude_known, a, s));
    const int grid = p.wgs * p.nblk;
    ProfScope ps(m, AAE_K_RANK, s);
    for (int g = 0; g * kFullSlots < max_truth; ++g) {      // 8 held-out items a row and round
        hipLaunchKernelGGL(rank_full_setup_kernel, dim3(p.rows), dim3(64), 0, s, tv, m->N, g, p.tgt_i, p.tgt_v, p.tcount);
        LAUNCHCHK("rank_full_setup");
        TRY(launch_rank(a, m->fused_nb, 1, kRankPick, grid, s));
        TRY(launch_rank(a, m->fused_nb, 1, kRankCount, grid, s));
        hipLaunchKernelGGL(rank_full_finish_kernel, dim3(p.rows), dim3(256), 0, s, tv, g, p.tgt_i, p.tcount,
                           reinterpret_cast<int*>(ranks_out));
        LAUNCHCHK("rank_full_finish");
    }
    return AAE_OK;
}

// the chunks loss_targets_kernel cuts the target rows into: kLossChunk entries each, by the longest row (0: not given)
int loss_chunks(int max_row_nnz) {
    return max_row_nnz > 0 ? std::max(1, std::min(kLossChunksMax, (max_row_nnz + kLossChunk - 1) / kLossChunk)) : kLossChunksMax;
}

// dh2 (workspace) of `rows` rows -> row_bce [rows]: the sum over the items of the row's cell losses against its targets `tv`
// (loss_eval.h).  The mask of the plan holds the TARGET entries: the loss epilogue skips them, loss_targets charges them.
int loss_from_dh2(aae_model* m, const RankPlan& p, const BatchView& tv, int max_row_nnz, double* row_bce_out, hipStream_t s) {
    RankArgs a;
    TRY(rank_mask_and_args(m, p, tv, 1, a, s));
    const int chunks = loss_chunks(max_row_nnz);
    ProfScope ps(m, AAE_K_RANK, s);
    TRY(launch_rank(a, m->fused_nb, 1, kRankLoss, p.wgs * p.nblk, s));
    hipLaunchKernelGGL(pick_loss_targets(), dim3(p.rows, chunks), dim3(256), 0, s, tv, (const float*)p.dh2, m->ldh,
                       (const float*)m->P[P_V3].p, m->ldh, m->h + 1, m->N, m->bf16 ? 1 : 0, p.csum);
    LAUNCHCHK("loss_targets");
    hipLaunchKernelGGL(pick_loss_finish(), dim3((p.rows + 255) / 256), dim3(256), 0, s, (const double*)p.lpart, p.wgs,
                       (const double*)p.csum, chunks, p.rows, row_bce_out);
    LAUNCHCHK("loss_finish");
    return AAE_OK;
}
// [mu | logvar] of `rows` rows -> row_kl [rows]
int loss_kl_rows(const float* mulv, int ld, int nc, int rows, double* row_kl_out, hipStream_t s) {
    hipLaunchKernelGGL(pick_vae_kl_rows(), dim3((rows + 3) / 4), dim3(256), 0, s, mulv, ld, nc, rows, row_kl_out);
    LAUNCHCHK("vae_kl_rows");
    return AAE_OK;
}
// the model's dense form: the LOGITS of the m->rows rows of the call in the [max_batch][n_items] scratch -> row_bce
int loss_rows_dense(aae_model* m, const BatchView& tv, double* row_bce_out, hipStream_t s) {
    ProfScope ps(m, AAE_K_RANK, s);
    hipLaunchKernelGGL(pick_loss_rows_dense(), dim3(m->rows), dim3(256), 0, s, m->G.p, m->ldn, m->N, tv, row_bce_out);
    LAUNCHCHK("loss_rows_dense");
    return AAE_OK;
}

// ---- the dense form, written once: a [rows][ld] score matrix of fp32 or int32 -> lists / ranks -----------------------------
// The only launches of rank_long_dense_kernel / rank_full_dense_kernel: behind the model's calls (below) and the handle-free
// baselines (abi_cooc.h, abi_lowrank.h).  known: the rows' known items (masked in place when exclude_known); truth: the rows'
// held-out items.  The scores are overwritten where a known item is masked.
template <class SC>
int dense_topk(SC* scores, int64_t ld, int n_items, const BatchView& known, int rows, int k, int exclude_known, int32_t* idx_out,
               float* val_out, hipStream_t s) {
    hipLaunchKernelGGL(pick_rank_long_dense<SC>(), dim3(rows), dim3(kLongNT), 0, s, scores, (int)ld, n_items, known, exclude_known, k,
                       reinterpret_cast<int*>(idx_out), val_out);
    LAUNCHCHK("rank_long_dense");
    return AAE_OK;
}
template <class SC>
int dense_ranks(SC* scores, int64_t ld, int n_items, const BatchView& known, const BatchView& truth, int rows, int exclude_known,
                int32_t* ranks_out, hipStream_t s) {
    hipLaunchKernelGGL(pick_rank_full_dense<SC>(), dim3(rows), dim3(kFullNT), 0, s, scores, (int)ld, n_items, known, truth, 0,
                       exclude_known, reinterpret_cast<int*>(ranks_out));
    LAUNCHCHK("rank_full_dense");
    return AAE_OK;
}

// the model's dense form: the m->rows rows of the call, their scores in the [max_batch][n_items] scratch
int rank_full_dense(aae_model* m, const BatchView& bv, const BatchView& tv, int exclude_known, int32_t* ranks_out, hipStream_t s) {
    ProfScope ps(m, AAE_K_RANK, s);
    return dense_ranks(m->G.p, m->ldn, m->N, bv, tv, m->rows, exclude_known, ranks_out, s);
}

// the decoder's hidden layers of a chain program whose slot `src` holds [z | condition head] (and slot 5 the rest of a wide
// input): -> p.dh2
void rank_dec_hidden(aae_model* m, ChainBuilder& cb, int srcA, int srcB, int rows, const RankPlan& p, hipStream_t s) {
    const int h = m->h;
    ChainOp& v1 = add_dec_in_fwd(cb, m, srcA, srcB, 3, s);
    v1.d = make_drop(m, 0, false, nullptr, nullptr, rows, h, 2); v1.one_col = h;
    ChainOp& v2 = cb.add(cop_fwd(m, P_V2, 3, 4, h + 1, h, CEPI_DROPACT, s));
    v2.d = make_drop(m, 1, false, nullptr, nullptr, rows, h, 3); v2.one_col = h; cop_out(v2, p.dh2, m->ldh);
}

BatchView rank_view(const aae_batch* b) {
    BatchView bv;
    bv.indptr = b->indptr_dev; bv.indices = b->indices_dev; bv.values = b->values_dev;
    bv.rows = b->rows_dev; bv.row_start = b->row_start; bv.n_rows = b->n_rows;
    return bv;
}

// the first layer of a rank call: a1 / eh1 [rows][ldh] = (act of) enc.lin1 of the rows, eval mode; every deferred launch joined
int rank_first_layer(aae_model* m, const aae_batch* batch, float* a1, float* eh1, float* rscale, hipStream_t s) {
    const int rows = batch->n_rows, h = m->h;
    TRY(join_deferred(m, s));
    if (m->flushed_hstep != m->hstep) {     // every row of enc.lin1 through the current step: once after the last training step
        TRY(lazy_flush(m, s));               // (rows fall behind only when a step opens: hstep counts them)
        m->flushed_hstep = m->hstep;
    }
    DropSpec d1 = make_drop(m, 0, false, nullptr, nullptr, rows, h, 0);
    ProfScope ps(m, AAE_K_ENC_GATHER, s);
    hipLaunchKernelGGL(enc_gather_kernel, dim3(rows), dim3(1024), (uint32_t)((size_t)16 * r4(h) * sizeof(float)), s, rank_view(batch),
                       (const float*)m->P[P_W1T].p, m->ldw1, (const float*)m->P[P_B1].p, h, (int)m->cfg.normalize_inputs,
                       a1, eh1, m->ldh, (int)m->cfg.activation, d1, (uint64_t)m->cfg.seed, (const long long*)m->step_ctr,
                       rscale, (const float*)nullptr, AdvanceJob{nullptr, nullptr, nullptr, nullptr, 0}, (long long)-1);
    LAUNCHCHK("enc_gather (rank)");
    return AAE_OK;
}

// the rows' forward pass up to the decoder's last hidden layer -> p.dh2 (eval mode: no dropout; aae.py:840-870)
int rank_predict_hidden(aae_model* m, const aae_batch* batch, const float* cond_dev, const RankPlan& p, hipStream_t s) {
    const int rows = batch->n_rows, h = m->h, c = m->c, cp = m->cp;
    TRY(rank_first_layer(m, batch, p.a1, p.eh1, p.rscale, s));
    ChainBuilder cb(m, rows);
    ChainOp& l = cb.add(cop_load(p.eh1, m->ldh, 0, h)); l.one_col = h;
    ChainOp& w2 = cb.add(cop_fwd(m, P_W2, 0, 1, h + 1, h, CEPI_DROPACT, s));
    w2.d = make_drop(m, 1, false, nullptr, nullptr, rows, h, 1); w2.one_col = h;
    cb.add(cop_fwd(m, P_W3, 1, 2, h + 1, c, CEPI_NONE, s));
    ChainOp& f = m->cfg.enc_final == AAE_FINAL_LINEAR ? cb.P.ops[cb.P.nops - 1] : cb.add(cop(COP_FINAL_FWD, 2, 2, c));
    f.aux = m->cfg.enc_final;
    if (wide_dec_in(m)) {
        const int nA = kCWide - c, ci = m->cfg.cond_inc;
        ChainOp& ca = cb.add(cop_load(cond_dev, ci, 2, nA)); ca.dst_col0 = c;
        ChainOp& cl = cb.add(cop_load(cond_dev + nA, ci, 5, ci - nA)); cl.one_col = cp - kCWide;
    } else if (m->cfg.cond_inc > 0) {
        ChainOp& cl = cb.add(cop_load(cond_dev, m->cfg.cond_inc, 2, m->cfg.cond_inc)); cl.dst_col0 = c; cl.one_col = cp;
    } else {
        f.one_col = cp;
    }
    rank_dec_hidden(m, cb, 2, 5, rows, p, s);
    return launch_chain(m, cb, s);
}

// the same from a decoder input the caller built: zc_dev [rows][zc_ld] -> p.dh2
int rank_decode_hidden(aae_model* m, const float* zc_dev, int64_t zc_ld, int rows, const RankPlan& p, hipStream_t s) {
    const int cp = m->cp;
    TRY(join_deferred(m, s));
    ChainBuilder cb(m, rows);
    if (wide_dec_in(m)) {
        cb.add(cop_load(zc_dev, (int)zc_ld, 2, kCWide));
        ChainOp& lb = cb.add(cop_load(zc_dev + kCWide, (int)zc_ld, 5, cp - kCWide)); lb.one_col = cp - kCWide;
    } else {
        ChainOp& l = cb.add(cop_load(zc_dev, (int)zc_ld, 2, cp)); l.one_col = cp;
    }
    rank_dec_hidden(m, cb, 2, 5, rows, p, s);
    return launch_chain(m, cb, s);
}

// k > 32, the dense form: [rows][ldn] scores in the scratch -> [rows][k]
int rank_long_dense(aae_model* m, int k, int exclude_known, int32_t* idx_out, float* val_out, hipStream_t s) {
    ProfScope ps(m, AAE_K_RANK, s);
    return dense_topk(m->G.p, m->ldn, m->N, m->bv, m->rows, k, exclude_known, idx_out, val_out, s);
}

// After a fused k > 32 call over plan `p`: the rows' entry counts (synchronises `s`), the handle's statistics, and the spans
// of at most max_batch rows that hold a row whose list overflowed - the caller ranks those through the score matrix.
int rank_long_overflow(aae_model* m, const aae_batch* b, const RankPlan& p, hipStream_t s, std::vector<std::pair<int, int>>& spans) {
    const int rows = b->n_rows;
    // (a span keeps to the dense path's per-batch bounds: max_batch rows, max_nnz entries)
    const int span = std::max(1, std::min(m->R, b->max_row_nnz > 0 ? m->cfg.max_nnz / b->max_row_nnz : m->R));
    std::vector<int> cnt(rows);
    HIPCHK(hipMemcpyAsync(cnt.data(), p.count, (size_t)rows * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    m->long_stats[0] += 1; m->long_stats[1] += rows;
    spans.clear();
    for (int r = 0; r < rows; ++r) {
        m->long_stats[3] += cnt[r]; m->long_stats[4] = std::max<int64_t>(m->long_stats[4], cnt[r]);
        if (cnt[r] <= p.cap) continue;
        m->long_stats[2] += 1;
        if (spans.empty() || r >= spans.back().first + spans.back().second) spans.push_back({r, std::min(span, rows - r)});
    }
    return AAE_OK;
}

// The rows of a model's ranking call.  zc != NULL: the decode form - a caller-built decoder input (code | imposed conditions
// of any plugin kind), the second half of predict (aae.py:855-866); `batch` names the input rows whose items are excluded and
// cond / eps are not read.
struct RankInput {
    aae_batch batch;
    const float* cond;          // predict form: [rows][cond_inc] (NULL without a condition)
    const float* eps;           // ... of the aae_vae_* calls: [rows][n_code] (NULL: the counter generator, rows counted from grow0)
    const float* zc; int64_t zc_ld;
    int grow0;                  // the generator row of row 0
    bool vae;                   // the aae_vae_* family was called (its checks have seen a VAE handle)
};

// rows [off, off + n) of a call as a call of their own, within the per-batch bounds of the dense path: the one place that
// knows the strides of a call's inputs
RankInput rank_cut(const aae_model* m, const RankInput& in, int off, int n) {
    RankInput c = in;
    aae_batch& b = c.batch;
    if (b.rows_dev) b.rows_dev += off; else b.row_start += off;
    b.n_rows = n; b.generation = 0;
    if (b.max_row_nnz > 0) b.nnz_bound = (int32_t)std::min<int64_t>((int64_t)n * b.max_row_nnz, b.nnz_bound);
    const size_t r0 = (size_t)off;
    auto from_r0 = [r0](const float* p, size_t ld) { return p ? p + r0 * ld : nullptr; };
    c.cond = from_r0(c.cond, m->cfg.cond_inc); c.eps = from_r0(c.eps, m->c); c.zc = from_r0(c.zc, c.zc_ld);
    c.grow0 += off;
    return c;
}

// ---- argument checks of every ranking entry point, the handle-free ones included: `who` (the entry point) opens the message ----
int rank_check_batch(const char* who, const aae_batch* b) {
    if (!b || !b->indptr_dev || !b->indices_dev || !b->values_dev) return fail(AAE_EINVAL, std::string(who) + ": batch pointers are NULL");
    return AAE_OK;
}
int rank_check_k(const char* who, int k, int n_items) {
    if (k < 1 || k > kLongKMax || k > n_items) return fail(AAE_EINVAL, std::string(who) + ": k must be in [1, min(1024, n_items)]");
    return AAE_OK;
}
int rank_check_lists(const char* who, const int32_t* idx_out_dev, const float* val_out_dev) {
    if (!idx_out_dev || !val_out_dev) return fail(AAE_EINVAL, std::string(who) + ": idx_out_dev / val_out_dev is NULL");
    return AAE_OK;
}
// the ground truth of a full-ranking call: the `n_rows` rows of the call, one for one (its values are not read)
int rank_check_truth(const char* who, int n_rows, const aae_batch* truth) {
    const std::string w(who);
    if (!truth || !truth->indptr_dev || !truth->indices_dev) return fail(AAE_EINVAL, w + ": truth pointers are NULL");
    if (truth->n_rows != n_rows) return fail(AAE_EINVAL, w + ": truth names another number of rows than the call's input rows");
    return AAE_OK;
}

// The one check of the model's ranking entry points - the eight calls and the four *_max_rows.  form: what the entry point
// takes; ptrs: its handle and every pointer that must not be NULL were given; k: NULL for a full-ranking call, which names
// its truth rows instead.  Nothing is launched before it passes.
enum { kRankFormRows, kRankFormPredict, kRankFormDecode };      // (rows: a *_max_rows call - no batch)
int rank_check_call(const char* who, const aae_model* m, bool vae, int form, bool ptrs, const int32_t* k, const float* cond_dev,
                    const float* eps_dev, int64_t zc_ld, const aae_batch* batch, const aae_batch* truth) {
    const std::string w(who);
    if (!m || !ptrs) return fail(AAE_EINVAL, w + ": NULL argument");
    if (vae && (!m->vae || !(m->use_chain || m->vae_layers))) return fail(AAE_ESTATE, w + ": model was not created in VAE mode (cfg.model_kind = 3)");
    auto predict_args = [&]() {
        if (m->cfg.cond_inc > 0 && !cond_dev) return fail(AAE_EINVAL, w + ": cond_inc > 0 needs cond_dev");
        if (vae && m->cfg.rng_mode == AAE_RNG_INJECT && !eps_dev) return fail(AAE_EINVAL, w + ": rng_mode inject needs eps_dev");
        return AAE_OK;
    };
    // (the aae_vae_* calls name a missing cond / eps before a k out of range, the aae_* calls behind it)
    if (form == kRankFormPredict && vae) TRY(predict_args());
    if (k) TRY(rank_check_k(who, *k, m->N));
    if (form == kRankFormPredict && !vae) TRY(predict_args());
    if (form == kRankFormRows) return AAE_OK;
    if (form == kRankFormDecode && zc_ld < m->cp) return fail(AAE_EINVAL, w + ": zc_ld < n_code + cond_inc");
    TRY(rank_check_batch(who, batch));
    if (k) return AAE_OK;
    TRY(rank_check_truth(who, batch->n_rows, truth));
    if (truth->max_row_nnz < 1) return fail(AAE_EINVAL, w + ": truth needs max_row_nnz: the entries of its longest row (an upper bound)");
    return AAE_OK;
}

// ---- the VAE's form (aae_vae_predict_topk / _ranks / _decode_topk / _decode_ranks; reference vae.py:229-266) -------------
// The same workspace, the same ranking passes over dec.lin3 (= fc4); the hidden half is the VAE's forward in ONE program on the
// 4-row kernel: eh1 -> [mu | logvar] = [fc21; fc22] eh1 -> z = mu + eps * exp(logvar / 2) -> condition block -> dh2 = act(fc3 zc).

// the F4 copies from the parameters as they stand (behind join_deferred: nothing else writes or reads the scratch)
int vae_rank_derive(aae_model* m, const VaeRankCopies& c, hipStream_t s) {
    HIPCHK(hipMemsetAsync(c.w3, 0, c.floats * sizeof(float), s));      // (the k-chunks beyond a matrix read as zero, not as what a step left)
    for (int pid : {P_W3, P_V1}) {
        const Ten& W = m->P[pid];
        hipLaunchKernelGGL(interleave4_kernel, dim3(grid1d((size_t)W.rows * ((W.cols + 3) / 4))), dim3(256), 0, s, W.p, (int)W.ld,
                           W4Copies{pid == P_W3 ? c.w3 : c.v1, c.d4, (int)W.rows, (int)W.cols, nullptr, nullptr, nullptr, kCWide});
        LAUNCHCHK("interleave4 (vae rank)");
    }
    return AAE_OK;
}

// a forward layer of the VAE's rank program: cop_fwd with the workspace's F4 copy
ChainOp vae_cop_fwd(const aae_model* m, int pid, const float* w4, int src, int dst, int K, int N, int epi) {
    ChainOp o = cop_linear(COP_LINEAR, src, dst, m->P[pid], K, N, epi);
    o.W4 = w4; o.ns4 = (int)m->P[pid].rows;
    return o;
}

// the decoder half: slot 2 holds [z | condition | 1], or the first 208 columns of a wider input whose later k-parts come from
// g (add_vae_dec_in_fwd) through slot 4 -> dh2 = act(fc3 zc) (no dropout in the VAE: the DropSpec stays disabled)
void vae_rank_dec_hidden(aae_model* m, ChainBuilder& cb, const VaeRankCopies& c, const float* g, int ldg, int g_col0, float* dh2) {
    ChainOp& v1 = add_vae_dec_in_fwd(cb, m, g, ldg, g_col0, false, 2, 4, 3, c.v1);
    v1.one_col = m->h; cop_out(v1, dh2, m->ldh);
}

// rows of `batch` -> dh2 [rows][ldh].  eps_dev: row 0 of the batch (NULL: the counter generator, rows counted from grow0);
// a1 / eh1 / rscale: [rows] scratch of the first layer
// mulv: where a loss call keeps [mu | logvar] [rows][2 n_code] for its KL term (NULL: nobody reads them)
int vae_rank_predict_hidden(aae_model* m, const aae_batch* batch, const float* cond_dev, const float* eps_dev, int grow0,
                            const VaeRankCopies& c, float* a1, float* eh1, float* rscale, float* dh2, hipStream_t s,
                            float* mulv = nullptr) {
    const int rows = batch->n_rows, h = m->h, nc = m->c, cp = m->cp;
    TRY(rank_first_layer(m, batch, a1, eh1, rscale, s));
    TRY(vae_rank_derive(m, c, s));
    ChainBuilder cb(m, rows);
    cb.vae4 = true;
    ChainOp& l = cb.add(cop_load(eh1, m->ldh, 0, h)); l.one_col = h;
    ChainOp& ml = cb.add(vae_cop_fwd(m, P_W3, c.w3, 0, 1, h + 1, 2 * nc, CEPI_NONE));
    if (mulv) cop_out(ml, mulv, 2 * nc);
    ChainOp& rp = cb.add(cop(COP_REPARAM, 1, 2, nc));
    rp.W = eps_dev; rp.ldw = nc; rp.aux = 12; rp.grow0 = grow0;        // (stream id 12: chain_vae_forward's draws)
    if (wide_dec_in(m)) {
        ChainOp& ca = cb.add(cop_load(cond_dev, m->cfg.cond_inc, 2, kCWide - nc)); ca.dst_col0 = nc;
    } else if (m->cfg.cond_inc > 0) {
        ChainOp& cl = cb.add(cop_load(cond_dev, m->cfg.cond_inc, 2, m->cfg.cond_inc)); cl.dst_col0 = nc; cl.one_col = cp;
    } else {
        rp.one_col = cp;
    }
    vae_rank_dec_hidden(m, cb, c, cond_dev, m->cfg.cond_inc, nc, dh2);
    return launch_chain(m, cb, s);
}

// the same from a decoder input the caller built: zc_dev [rows][zc_ld] -> dh2
int vae_rank_decode_hidden(aae_model* m, const float* zc_dev, int64_t zc_ld, int rows, const VaeRankCopies& c, float* dh2, hipStream_t s) {
    TRY(join_deferred(m, s));
    TRY(vae_rank_derive(m, c, s));
    ChainBuilder cb(m, rows);
    cb.vae4 = true;
    ChainOp& l = cb.add(cop_load(zc_dev, (int)zc_ld, 2, std::min(m->cp, kCWide)));
    if (!wide_dec_in(m)) l.one_col = m->cp;
    vae_rank_dec_hidden(m, cb, c, zc_dev, (int)zc_ld, 0, dh2);
    return launch_chain(m, cb, s);
}

// ---- the hidden half of a fused call, either kind of handle, either form: rows of `in` -> w.p.dh2 [rows][ldh] (w.p.a1 / eh1 /
// rscale: [rows] scratch of the predict form's first layer) ---------------------------------------------------------------
int rank_hidden(aae_model* m, const RankInput& in, const RankWs& w, hipStream_t s) {
    const RankPlan& p = w.p;
    const int rows = in.batch.n_rows;
    if (!in.vae) return in.zc ? rank_decode_hidden(m, in.zc, in.zc_ld, rows, p, s) : rank_predict_hidden(m, &in.batch, in.cond, p, s);
    if (in.zc) return vae_rank_decode_hidden(m, in.zc, in.zc_ld, rows, w.c, p.dh2, s);
    return vae_rank_predict_hidden(m, &in.batch, in.cond, in.eps, in.grow0, w.c, p.a1, p.eh1, p.rscale, p.dh2, s, p.mulv);
}

// A span of a fused k > 32 aae_vae_* call that holds a row whose collect list overflowed: the rows of `sub` (<= max_batch)
// -> their scores in the scratch.  The hidden half runs the fused call's own program on the handle's per-batch buffers - the
// same eps rows (eps / generator rows from grow0), the same dh2 bits - then fc4 + sigmoid into the scratch, which the copies'
// head is part of: they are derived again per span.
int vae_span_scores(aae_model* m, const RankInput& sub, hipStream_t s) {
    TRY(set_batch(m, &sub.batch));
    RankWs w; memset(&w, 0, sizeof(w));
    w.c = vae_rank_copies(m, m->G.p);
    w.p.a1 = m->a1.p; w.p.eh1 = m->eh1.p; w.p.rscale = m->rscale; w.p.dh2 = m->dh2.p;
    TRY(rank_hidden(m, sub, w, s));
    EpiSigmoid e; e.out = m->G.p; e.ld = m->ldn;
    return linear_fwd(m->dh2.p, m->ldh, m->rows, m->P[P_V3], e, s, gmode(m));
}

}  // namespace
