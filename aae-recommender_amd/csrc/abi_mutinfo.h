// Entry points of the mutual information of an unstored contingency table (mutinfo.h): the marginals, the row pass, the finish.
// Handle-free like the spgemm calls, and on the same operands: every buffer is the caller's, every launch (and the memsets that
// zero the integer marginals) goes to the caller's stream, nothing synchronises.  u_dev is aae_spgemm_i32_bound's.
// (one of the parts of aae_abi.hip's translation unit: included there in order, not on its own)
#pragma once

extern "C" {

int aae_mi_i32_marginals(const aae_cooc* A, const aae_cooc* B, int32_t p, int32_t n, int64_t* a_dev, int64_t* pj_dev,
                         double* lnpj_dev, void* stream) {
    if (!a_dev || !pj_dev || !lnpj_dev) return fail(AAE_EINVAL, "aae_mi_i32_marginals: a_dev / pj_dev / lnpj_dev is NULL");
    TRY(spgemm_check("aae_mi_i32_marginals", A, B, n, a_dev));
    if (p < 0 || p > B->n_rows) return fail(AAE_EINVAL, "aae_mi_i32_marginals: p must be in [0, rows of B]");
    hipStream_t s = S(stream);
    if ((p > 0 && hipMemsetAsync(a_dev, 0, (size_t)p * sizeof(int64_t), s) != hipSuccess) ||
        (n > 0 && hipMemsetAsync(pj_dev, 0, (size_t)n * sizeof(int64_t), s) != hipSuccess))
        return fail(AAE_EHIP, "aae_mi_i32_marginals: hipMemsetAsync failed");
    if (n == 0) return AAE_OK;
    if (p > 0 && A->n_rows > 0) {
        const CoocView a{A->indptr_dev, A->indices_dev, A->values_dev, A->n_rows}, b{B->indptr_dev, B->indices_dev, B->values_dev, B->n_rows};
        hipLaunchKernelGGL(pick_mi_colsum(), dim3(kMiBlocks), dim3(kMiNT), 0, s, a, (int)p, reinterpret_cast<unsigned long long*>(a_dev));
        LAUNCHCHK("mi_colsum");
        hipLaunchKernelGGL(pick_mi_pj(), dim3((unsigned)(((int64_t)p + kMiNT / 64 - 1) / (kMiNT / 64))), dim3(kMiNT), 0, s, b, (int)p, (int)n,
                           reinterpret_cast<const unsigned long long*>(a_dev), reinterpret_cast<unsigned long long*>(pj_dev));
        LAUNCHCHK("mi_pj");
    }
    hipLaunchKernelGGL(pick_mi_lnpj(), dim3((unsigned)(((int64_t)n + kMiNT - 1) / kMiNT)), dim3(kMiNT), 0, s, pj_dev, (int)n, lnpj_dev);
    LAUNCHCHK("mi_lnpj");
    return AAE_OK;
}

int aae_mi_i32_rows(const aae_cooc* A, const aae_cooc* B, int32_t n, const int64_t* u_dev, const double* lnpj_dev,
                    double* row_s1_dev, int64_t* row_pi_dev, void* stream) {
    TRY(spgemm_check("aae_mi_i32_rows", A, B, n, u_dev));
    if (!lnpj_dev || !row_s1_dev || !row_pi_dev) return fail(AAE_EINVAL, "aae_mi_i32_rows: lnpj_dev / row_s1_dev / row_pi_dev is NULL");
    if (A->n_rows == 0) return AAE_OK;
    MiRowArgs g{};
    g.A = CoocView{A->indptr_dev, A->indices_dev, A->values_dev, A->n_rows};
    g.B = CoocView{B->indptr_dev, B->indices_dev, B->values_dev, B->n_rows};
    g.p = B->n_rows; g.n = n; g.u = u_dev;
    g.lnpj = lnpj_dev; g.row_s1 = row_s1_dev; g.row_pi = row_pi_dev;
    hipStream_t s = S(stream);
    hipLaunchKernelGGL(pick_mi_hash(), dim3((unsigned)g.A.n_rows), dim3(kSpgemmHashNT), 0, s, g);
    LAUNCHCHK("mi_hash");
    hipLaunchKernelGGL(pick_mi_tile(), dim3((unsigned)g.A.n_rows), dim3(kSpgemmTileNT), 0, s, g);
    LAUNCHCHK("mi_tile");
    return AAE_OK;
}

int aae_mi_i32_finish(int32_t m, const double* row_s1_dev, const int64_t* row_pi_dev, void* out_dev, void* stream) {
    if (m < 0) return fail(AAE_EINVAL, "aae_mi_i32_finish: m is negative");
    if (!row_s1_dev || !row_pi_dev || !out_dev) return fail(AAE_EINVAL, "aae_mi_i32_finish: a pointer is NULL");
    if ((reinterpret_cast<uintptr_t>(out_dev) & 7) != 0) return fail(AAE_EINVAL, "aae_mi_i32_finish: out_dev must be 8-byte aligned");
    hipLaunchKernelGGL(pick_mi_finish(), dim3(1), dim3(kMiFinishNT), 0, S(stream), (int)m, row_s1_dev, row_pi_dev, out_dev);
    LAUNCHCHK("mi_finish");
    return AAE_OK;
}

}  // extern "C"
