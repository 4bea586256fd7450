// Every templated kernel family of the library, spelled ONCE: pick_*() maps run-time values to a typed kernel pointer,
// each_*() hands out the members a handle may launch (aae_create raises their dynamic-LDS limit through it).
// (one of the parts of aae_abi.hip's translation unit: included there behind the kernel headers, not on its own)
// A picker returns nullptr for a combination that is not compiled (`if constexpr`: asking for it does not instantiate it) and
// its caller fails with AAE_ESTATE - nothing falls through to another member.  An enumeration walks its picker over the whole
// run-time domain, so a new template flag is one more argument here and nowhere else.
#pragma once

#include <type_traits>

namespace {

using DecKernel = void (*)(DecFusedArgs);
using RankKernel = void (*)(RankArgs);
using ChainKernel = void (*)(ChainProgram);
using MergeKernel = void (*)(const float*, const int*, const float*, int, int, int, int*, float*);

// run-time x -> f(integral_constant<V>) for the V of the list that equals x; nullptr for any other x
template <class R, int... Vs, class F>
R pick_of(int x, F&& f) {
    R r = nullptr;
    (void)(... || (x == Vs && ((r = f(std::integral_constant<int, Vs>{})), true)));
    return r;
}
// run-time bools -> f(bool_constant...), in the order given
template <class R, bool... Bs, class F>
R pick_flags(F&& f) { return f(std::bool_constant<Bs>{}...); }
template <class R, bool... Bs, class F, class... Rest>
R pick_flags(F&& f, bool b, Rest... rest) {
    return b ? pick_flags<R, Bs..., true>(f, rest...) : pick_flags<R, Bs..., false>(f, rest...);
}
// NB = ceil((h + 1) / 16) column blocks of the hidden width (aae_model::fused_nb); K = list entries per workgroup (rank_K)
template <class R, class F> R pick_nb(int nb, F&& f) { return pick_of<R, 4, 7, 13>(nb, f); }
template <class R, class F> R pick_k(int k, F&& f) { return pick_of<R, 10, 20, 32>(k, f); }
constexpr int kPickNb[] = {4, 7, 13}, kPickK[] = {10, 20, 32};
#define NB_ decltype(NB)::value      // (an enclosing lambda's constant, named without capturing it)

template <class K>
bool raise_lds_limit(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

// ---- the single launch of the output layer: dec_fused.h with its moving-window form; dec_fused_bf16.h (no window form)
inline DecKernel pick_dec_fused(int nb, bool win) {
    return pick_nb<DecKernel>(nb, [&](auto NB) { return pick_flags<DecKernel>([](auto WIN) -> DecKernel { return dec_fused_kernel<NB_, WIN()>; }, win); });
}
inline DecKernel pick_dec_fused_bf16(int nb) {
    return pick_nb<DecKernel>(nb, [](auto NB) -> DecKernel { return dec_fused_bf16_kernel<NB_>; });
}
template <class F> void each_dec_fused(F&& f) { for (int nb : kPickNb) for (int win = 0; win < 2; ++win) f(pick_dec_fused(nb, win)); }
template <class F> void each_dec_fused_bf16(F&& f) { for (int nb : kPickNb) f(pick_dec_fused_bf16(nb)); }

// ---- dec_crit_x3.h: the split forms.  ONE = the handle is a bf16 one; TS (the debug timelines) exists for NB == 13 alone, three-term, no window
inline DecKernel pick_dec_crit_x3(int nb, bool ts, bool one, bool win) {
    return pick_nb<DecKernel>(nb, [&](auto NB) { return pick_flags<DecKernel>([](auto TS, auto ONE, auto WIN) -> DecKernel {
        if constexpr (TS() && (NB_ != 13 || ONE() || WIN())) return nullptr; else return dec_crit_x3_kernel<NB_, TS(), ONE(), WIN()>; }, ts, one, win); });
}
inline DecKernel pick_dec_opt_x3(int nb, bool one, bool win) {
    return pick_nb<DecKernel>(nb, [&](auto NB) { return pick_flags<DecKernel>([](auto ONE, auto WIN) -> DecKernel {
        return dec_opt_x3_kernel<NB_, ONE(), WIN()>; }, one, win); });
}
inline DecKernel pick_dec_opt_blocks_x3(int nb, bool ts, bool win) {
    return pick_nb<DecKernel>(nb, [&](auto NB) { return pick_flags<DecKernel>([](auto TS, auto WIN) -> DecKernel {
        if constexpr (TS() && (NB_ != 13 || WIN())) return nullptr; else return dec_opt_blocks_x3_kernel<NB_, TS(), WIN()>; }, ts, win); });
}
// (ONE: the handle's dtype - a bf16 handle launches the one-term members, an fp32 handle the three-term ones)
template <class F> void each_dec_crit_x3(bool one, F&& f) {
    for (int nb : kPickNb) for (int i = 0; i < 4; ++i) if (DecKernel k = pick_dec_crit_x3(nb, i & 1, one, i & 2)) f(k);
}
template <class F> void each_dec_opt_x3(bool one, F&& f) { for (int nb : kPickNb) for (int win = 0; win < 2; ++win) f(pick_dec_opt_x3(nb, one, win)); }
template <class F> void each_dec_opt_blocks_x3(F&& f) {
    for (int nb : kPickNb) for (int i = 0; i < 4; ++i) if (DecKernel k = pick_dec_opt_blocks_x3(nb, i & 1, i & 2)) f(k);
}

// ---- rank_x3.h.  Which of the two rank kernels keeps the lists of a (NB, K): the v2 wave mapping where its registers do
// not spill, rank_x3_kernel (the r4 mapping) for the other list sizes.  The choice is static, so each (NB, K) is compiled
// in the one form it is launched in.
constexpr bool rank_v2_nb(int nb, int K) { return K == 10 || (K == 20 && nb < 13); }
// a rank launch: the kernel, its dynamic LDS, and the name a launch error carries
struct RankPick { RankKernel kernel; size_t lds; const char* name; };
inline RankPick pick_rank_lists(int nb, int K, bool win) {
    const bool v2 = rank_v2_nb(nb, K);
    const RankKernel kernel = pick_nb<RankKernel>(nb, [&](auto NB) { return pick_k<RankKernel>(K, [&](auto KK) {
        return pick_flags<RankKernel>([](auto WIN) -> RankKernel {
            constexpr int K_ = decltype(KK)::value;
            if constexpr (rank_v2_nb(NB_, K_)) return rank_x3v2_kernel<NB_, K_, WIN()>; else return rank_x3_kernel<NB_, K_, WIN(), kRankLists>; }, win); }); });
    return {kernel, v2 ? rank_x3v2_lds_bytes(nb) : rank_x3_lds_bytes(nb), v2 ? "rank_x3v2" : "rank_x3"};
}
// K = 1 is the front end of the epilogues that keep no lists - collect (rank_long.h), pick and count (rank_full.h), loss
// (loss_eval.h): they exist with it alone, and it not without one of them
inline RankPick pick_rank_epilogue(int nb, int epi, bool win) {
    const RankKernel kernel = pick_nb<RankKernel>(nb, [&](auto NB) { return pick_of<RankKernel, kRankCollect, kRankPick, kRankCount, kRankLoss>(epi, [&](auto EPI) {
        return pick_flags<RankKernel>([](auto WIN) -> RankKernel { return rank_x3_kernel<NB_, 1, WIN(), decltype(EPI)::value>; }, win); }); });
    return {kernel, rank_x3_lds_bytes(nb), epi == kRankCollect ? "rank_x3 (collect)" : epi == kRankPick ? "rank_x3 (pick)" : epi == kRankCount ? "rank_x3 (count)" : "rank_x3 (loss)"};
}
inline MergeKernel pick_rank_merge(int K) {
    return pick_k<MergeKernel>(K, [](auto KK) -> MergeKernel { return rank_merge_kernel<KK()>; });
}
template <class F> void each_rank(F&& f) {
    for (int nb : kPickNb) for (int win = 0; win < 2; ++win) {
        for (int K : kPickK) f(pick_rank_lists(nb, K, win));
        for (int epi : {kRankCollect, kRankPick, kRankCount, kRankLoss}) f(pick_rank_epilogue(nb, epi, win));
    }
}

// ---- kernels.h: the register lists of the dense form, k <= 32 (K = rank_K(k)).  Static LDS: no limit to raise
using TopkRowsKernel = void (*)(float*, int, int, BatchView, int, int, int*, float*);
inline TopkRowsKernel pick_topk_rows(int K) {
    return pick_k<TopkRowsKernel>(K, [](auto KK) -> TopkRowsKernel { return topk_rows_kernel<KK()>; });
}

// ---- rank_long.h / rank_full.h, the dense forms, and cooc.h: one member per score type (DenseScore) - float, what every
// dense ranking call launches, and int32_t, the exact route of the co-occurrence baseline (abi_cooc.h aae_cooc_*_i32).  The
// type is the caller's matrix, so it is a template argument here and no run-time value.  Static LDS: no limit to raise
template <class SC> constexpr bool kDenseScoreType = std::is_same_v<SC, float> || std::is_same_v<SC, int32_t>;
template <class SC> using RankLongDenseKernel = void (*)(SC*, int, int, BatchView, int, int, int*, float*);
template <class SC> using RankFullDenseKernel = void (*)(SC*, int, int, BatchView, BatchView, int, int, int*);
template <class SC> using CoocScoresKernel = void (*)(CoocView, int, int, BatchView, SC*, long long);
template <class SC> inline RankLongDenseKernel<SC> pick_rank_long_dense() {
    static_assert(kDenseScoreType<SC>, "scores are fp32 or int32"); return rank_long_dense_kernel<SC>;
}
template <class SC> inline RankFullDenseKernel<SC> pick_rank_full_dense() {
    static_assert(kDenseScoreType<SC>, "scores are fp32 or int32"); return rank_full_dense_kernel<SC>;
}
template <class SC> inline CoocScoresKernel<SC> pick_cooc_scores() {
    static_assert(kDenseScoreType<SC>, "scores are fp32 or int32"); return cooc_scores_kernel<SC>;
}

// ---- chain.h (NM: the r6 activation classes, device_common.h act_fwd); chain4.h: the timeline in fp32 alone, the column
// form (a program without k-slices) in bf16 alone, the VAE's reparametrisation op in plain fp32 alone; chain16x3.h: the
// timeline in fp32 alone
inline ChainKernel pick_chain(bool bf, bool nm) {
    return pick_flags<ChainKernel>([](auto BF, auto NM) -> ChainKernel { return chain_kernel<BF(), NM()>; }, bf, nm);
}
inline ChainKernel pick_chain4(bool bf, bool ts, bool cols, bool vae = false) {
    return pick_flags<ChainKernel>([](auto BF, auto TS, auto COLS, auto VAE) -> ChainKernel {
        if constexpr ((TS() && (BF() || COLS())) || (COLS() && !BF()) || (VAE() && (BF() || TS() || COLS()))) return nullptr;
        else return chain4_kernel<BF(), TS(), COLS(), VAE()>; }, bf, ts, cols, vae);
}
inline ChainKernel pick_chain16x3(bool bf, bool ts) {
    return pick_flags<ChainKernel>([](auto BF, auto TS) -> ChainKernel {
        if constexpr (BF() && TS()) return nullptr; else return chain16x3_kernel<BF(), TS()>; }, bf, ts);
}
template <class F> void each_chain(bool nm, F&& f) { f(pick_chain(false, nm)); f(pick_chain(true, nm)); }
template <class F> void each_chain4(F&& f) { for (int i = 0; i < 8; ++i) if (ChainKernel k = pick_chain4(i & 1, i & 2, i & 4)) f(k); }
template <class F> void each_chain4_vae(F&& f) { f(pick_chain4(false, false, false, true)); }      // (a VAE handle's rank programs)
template <class F> void each_chain16x3(F&& f) { for (int i = 0; i < 4; ++i) if (ChainKernel k = pick_chain16x3(i & 1, i & 2)) f(k); }

// ---- vae_layers.h: the reparametrisation of a VAE handle on the per-layer route, forward and backward.  Static LDS: no limit to raise
inline auto pick_vae_reparam_fwd() { return vae_reparam_fwd_kernel; }
inline auto pick_vae_reparam_bwd() { return vae_reparam_bwd_kernel; }

// ---- gemm_f32.h for lowrank.h: the reconstruction scores = hidden . Vt^T on the fp32 matrix pipe - both operands k-contiguous
// (AT = 0, BT = 1), the streaming tile (16-deep slabs, 64 x 64), a plain store.  Static LDS: no limit to raise
using LowRankGemmKernel = void (*)(GemmShape, EpiStore);
inline LowRankGemmKernel pick_lowrank_gemm() { return gemm_f32_kernel<0, 1, 16, 64, EpiStore, false>; }

// ---- spgemm.h: the Count / Fill pair of each path.  Static LDS: no limit to raise
using SpgemmKernel = void (*)(SpgemmArgs);
inline SpgemmKernel pick_spgemm_hash(bool fill) {
    return pick_flags<SpgemmKernel>([](auto FILL) -> SpgemmKernel { return spgemm_hash_kernel<FILL()>; }, fill);
}
inline SpgemmKernel pick_spgemm_tile(bool fill) {
    return pick_flags<SpgemmKernel>([](auto FILL) -> SpgemmKernel { return spgemm_tile_kernel<FILL()>; }, fill);
}

// ---- sptrans.h: the Count pass, and the two launches of Fill (scatter, then the per-segment sort).  Static LDS: no limit to raise
using SptransKernel = void (*)(SptransArgs);
inline SptransKernel pick_sptrans_count() { return sptrans_count_kernel; }
inline SptransKernel pick_sptrans_scatter() { return sptrans_scatter_kernel; }
inline SptransKernel pick_sptrans_sort() { return sptrans_sort_kernel; }

// ---- mutinfo.h: the three marginal kernels, the row kernel of each spgemm path, the finish.  Static LDS: no limit to raise
using MiRowKernel = void (*)(MiRowArgs);
inline auto pick_mi_colsum() { return mi_colsum_kernel; }
inline auto pick_mi_pj() { return mi_pj_kernel; }
inline auto pick_mi_lnpj() { return mi_lnpj_kernel; }
inline MiRowKernel pick_mi_hash() { return mi_hash_kernel; }
inline MiRowKernel pick_mi_tile() { return mi_tile_kernel; }
inline auto pick_mi_finish() { return mi_finish_kernel; }

// ---- popular.h: the item counts, and lists / ranks from the one shared item order.  No LDS
inline auto pick_pop_counts() { return pop_counts_kernel; }
inline auto pick_pop_topk() { return pop_topk_kernel; }
inline auto pick_pop_ranks() { return pop_ranks_kernel; }

// ---- randrank.h: the random baseline's score block, lists (static LDS) and ranks (dynamic LDS below the default limit: none to raise)
inline auto pick_rand_scores() { return rand_scores_kernel; }
inline auto pick_rand_topk() { return rand_topk_kernel; }
inline auto pick_rand_ranks() { return rand_ranks_kernel; }

// ---- rank_metrics.h: per-row metric values from ranks, their (mean, std), ranks from lists.  Static LDS: no limit to raise
inline auto pick_metric_rows() { return metric_rows_kernel; }
inline auto pick_metric_finish() { return metric_finish_kernel; }
inline auto pick_ranks_from_lists() { return ranks_from_lists_kernel; }

// ---- loss_eval.h: the held-out loss behind the loss epilogue of rank_x3_kernel (above), its dense form, the VAE's KL rows.
// Static LDS: no limit to raise
inline auto pick_loss_targets() { return loss_targets_kernel; }
inline auto pick_loss_finish() { return loss_finish_kernel; }
inline auto pick_loss_rows_dense() { return loss_rows_dense_kernel; }
inline auto pick_vae_kl_rows() { return vae_kl_rows_kernel; }

// ---- lowrank.h: the CSR x row-major-dense product - the projection of the ranking calls and aae_spmm_f32 alike
using SpmmKernel = void (*)(LowRankView, BatchView, float*, long long);
inline SpmmKernel pick_lowrank_project() { return lowrank_project_kernel; }

// ---- cond_gather.h: the rows of the resident constant condition blocks.  One kernel - 16-byte or scalar is a per-block value
// of its argument, not a template flag.  No LDS
inline auto pick_cond_gather() { return cond_gather_kernel; }

#undef NB_
}  // namespace
