// Truncated-SVD scores (the reference's SVDRecommender, svd.py:15-57: predict = (X_test V^T) V[:, :n_items] with
// V = TruncatedSVD.components_ [dims][features], features = items (+ the tf-idf vocabulary of the titles)).  ONE fp32 table
// serves both products: Vt [features][ldv], row f = column f of V, ldv = dims rounded up to 4 floats, the padding zero.
//
//   projection       hidden[r][0:dims] = sum_e x_e * Vt[id_e][0:dims]        over the CSR entries e of feature row r
//   reconstruction   scores[r][j]      = sum_d hidden[r][d] * Vt[j][d]       j < n_items, fp32 [rows][ld] in HBM
//
//   lowrank_project_kernel   one workgroup per row, 64-256 threads (the host picks: one float4 of the table row per lane up to
//                            dims = 1024, up to four beyond - dims <= kProjDimsMax = 4096).  A row may hold thousands of
//                            entries (a bag plus its title words), so its ids and values go through LDS in pieces of
//                            kProjPiece = 256 entries; an id outside [0, n_features) is staged as (row 0, x = 0, table value
//                            replaced by 0): it adds nothing and nothing of the table reaches the sum.  Every lane then walks
//                            the piece IN CSR ORDER, one float4 load of the table row segment and four fmaf per entry and
//                            column group: hidden[r][d] is the k-ordered chain fmaf(x_e, Vt[id_e][d], acc) whatever the
//                            launch shape, so it carries the same bits from run to run and however the rows are chunked.
//                            A row without entries is a row of zeros.
//   reconstruction           gemm_f32_kernel<AT = 0, BT = 1, BK = 16, TS = 64, EpiStore> (gemm_f32.h; named in kernel_pick.h
//                            pick_lowrank_gemm): A = hidden (k contiguous), B = the first n_items rows of Vt (k contiguous),
//                            split-K count 1.  The arithmetic is the FP32 MATRIX PIPE (launch_gemm_mode's kGemmF32,
//                            v_mfma_f32_16x16x4_f32): every score is one k-ordered fp32 fmaf chain over d = 0 .. dims - 1
//                            that depends on its row of hidden and its row of Vt alone - the same bits however the rows are
//                            tiled or chunked.  No bf16 anywhere: inputs, products and sums are fp32.
//
// A-priori error bound (u = 2^-24, the unit roundoff of fp32; exact quantities: x, V in float64, h = x V^T, s = h V).
//   Vt and x are rounded to fp32 once (relative u each), the projection is a chain of nnz_r fmaf (Higham, Accuracy and
//   Stability of Numerical Algorithms, (3.5): relative gamma_n = n u / (1 - n u) against sum |x||V|), the reconstruction a
//   chain of dims fmaf over the computed hidden and the rounded table:
//       |scores[r][j] - s_rj|  <=  (dims + nnz_r + 4) u (1 + O(dims u)) * sum_d H_rd |V_dj|,   H_rd = sum_e |x_e| |V_d,id_e|
//   The tests hold the device to   tol_rj = 2^-23 (dims + nnz_r + 8) * sum_d |h_rd| |V_dj|   (c = 1: the fp32 pipe) - the same
//   count of roundings at twice the unit, against |h| instead of H >= |h|: a statement about the data as well (no heavy
//   cancellation inside a hidden unit), which the shapes of tests/test_lowrank_gpu.py are measured against.
// No atomics, no inline assembly.
#pragma once
#include "gemm_f32.h"
#include "kernels.h"

namespace aae {

constexpr int kProjDimsMax = 4096;      // widest hidden vector: four float4 per lane of a 256-thread workgroup
constexpr int kProjPiece = 256;         // entries of a row staged through LDS at a time
constexpr int kProjNV = 4;              // float4 column groups per lane at most

struct LowRankView { const float* vt; long long ldv; int n_features; int dims; };

// threads of the projection's workgroup: one lane per float4 of the (padded) hidden vector, whole waves, 256 at most
inline int lowrank_project_threads(int dims) {
    const int groups = (dims + 3) / 4;
    return groups >= 256 ? 256 : ((groups + 63) / 64) * 64;
}

__global__ __launch_bounds__(256) void lowrank_project_kernel(LowRankView V, BatchView bv, float* __restrict__ hidden, long long ldh) {
    __shared__ int s_id[kProjPiece];
    __shared__ float s_x[kProjPiece];
    const int tid = threadIdx.x, nt = blockDim.x, row = blockIdx.x;
    const int groups = (V.dims + 3) >> 2;           // float4 groups of a table row (ldv >= 4 * groups: all inside the row)
    float4 acc[kProjNV];
#pragma unroll
    for (int j = 0; j < kProjNV; ++j) acc[j] = make_float4(0.f, 0.f, 0.f, 0.f);
    const int dc = bv.doc(row);
    const int64_t lo = bv.indptr[dc], hi = bv.indptr[dc + 1];
    for (int64_t e0 = lo; e0 < hi; e0 += kProjPiece) {
        const int n = (int)(hi - e0 < (int64_t)kProjPiece ? hi - e0 : (int64_t)kProjPiece);
        __syncthreads();                            // (the piece before this one has been read by every lane)
        for (int i = tid; i < n; i += nt) {
            const int id = bv.indices[e0 + i];
            const bool ok = id >= 0 && id < V.n_features;
            s_id[i] = ok ? id : -1;
            s_x[i] = ok ? bv.values[e0 + i] : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int i = 0; i < n; ++i) {
            const int id = s_id[i];
            const float x = s_x[i];
            const float* p = V.vt + (size_t)(id < 0 ? 0 : id) * (size_t)V.ldv;
#pragma unroll
            for (int j = 0; j < kProjNV; ++j) {
                const int g = tid + j * nt;
                if (g < groups) {
                    float4 v = *reinterpret_cast<const float4*>(p + 4 * g);
                    if (id < 0) v = make_float4(0.f, 0.f, 0.f, 0.f);
                    acc[j].x = __builtin_fmaf(x, v.x, acc[j].x); acc[j].y = __builtin_fmaf(x, v.y, acc[j].y);
                    acc[j].z = __builtin_fmaf(x, v.z, acc[j].z); acc[j].w = __builtin_fmaf(x, v.w, acc[j].w);
                }
            }
        }
    }
    float* out = hidden + (size_t)row * (size_t)ldh;
#pragma unroll
    for (int j = 0; j < kProjNV; ++j) {
        const int g = tid + j * nt, c = 4 * g;
        if (g >= groups) continue;
        if (c + 3 < V.dims) { *reinterpret_cast<float4*>(out + c) = acc[j]; continue; }
        for (int i = 0; i < 4 && c + i < V.dims; ++i) out[c + i] = (&acc[j].x)[i];
    }
}

}  // namespace aae
