// The arithmetic of the layer-chain programs' non-linear ops, defined ONCE for the three interpreters (chain.h, chain4.h,
// chain16x3.h).  Each function works on values in registers and takes the op's pinned scalars as plain arguments: which
// thread holds which cell, how a slot is laid out, the loads, stores, barriers and the constant-1 column stay in the kernels.
// What the per-layer kernels share with these (prior_cell, adv_term, the activations) lives in device_common.h.
// Included by chain.h behind EpiCtx / chain_keep.
#pragma once

namespace aae {

// ---- the ACTBWD epilogue: v * act'(y) * (keep ? 1 / (1 - p) : 0), y = the forward activation of cell (grow, col) from
// wherever the caller keeps it (its slot format, a global row requested ahead).  NM as chain_epi.
template <bool NM>
__device__ __forceinline__ float chain_actbwd(const EpiCtx& c, int grow, int col, float v, float y) {
    v *= act_grad_from_y<NM>(c.act, y);
    if (c.den) v *= chain_keep(c, grow, col) ? c.mk : 0.f;
    return v;
}
// The same as ONE factor, for COP_SLABSUM's fused form, whose y comes from clamped reads over the whole slot row: outside
// the block's cells (cell == false) there is no mask / generator lookup - an injected mask ends with the batch's last row.
template <bool NM>
__device__ __forceinline__ float chain_actbwd_factor(const EpiCtx& c, int grow, int col, bool cell, float y) {
    const float kp = (c.den && cell) ? (chain_keep(c, grow, col) ? c.mk : 0.f) : 1.f;
    return act_grad_from_y<NM>(c.act, y) * kp;
}

// ---- VAE (vae.py:115-118): z = mu + eps * exp(logvar / 2); eps injected, or draw_gauss on the stream the op names
__device__ __forceinline__ float reparam_cell(float mu, float logvar, float eps) { return mu + eps * expf(0.5f * logvar); }
// its backward with the KL term's gradient (vae.py:132-145), one cell of [dL/dmu | dL/dlogvar]: gz = dL/dz of the cell's code
// column, scale = the step's gradient scale on the KL sum.  mu_half: the cell is dL/dmu - it also adds the column's KL term
// to kl; else it is dL/dlogvar (eps: the forward's draw, read by this half alone).
__device__ __forceinline__ float reparam_bwd_cell(bool mu_half, float gz, float mu, float lv, float eps, float scale, float& kl) {
    const float ev = expf(lv);
    if (mu_half) {
        kl += -0.5f * (1.f + lv - mu * mu - ev);
        return gz + scale * mu;
    }
    return gz * eps * 0.5f * expf(0.5f * lv) + scale * 0.5f * (ev - 1.f);
}

// ---- encoder output activation (PRIOR_ACTIVATIONS, aae.py:97-101), one wave per row of n <= 256 columns: a lane holds
// columns lane + 64 j, j < 4 (cells at columns >= n: any finite value, left as they are by kind 1).
// kind 1 softmax, 2 sigmoid, else identity.  Sums: a lane's columns ascending, then the wave.
__device__ __forceinline__ void final_act_fwd4(float (&z)[4], int n, int kind, int lane) {
    if (kind == 1) {
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (lane + 64 * j < n) mx = fmaxf(mx, z[j]);
        for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j) if (lane + 64 * j < n) { z[j] = expf(z[j] - mx); sum += z[j]; }
        sum = wave_sum(sum);
#pragma unroll
        for (int j = 0; j < 4; ++j) if (lane + 64 * j < n) z[j] = z[j] / sum;
    } else if (kind == 2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) z[j] = sigmoidf_(z[j]);
    }
}
// its backward: out = dL/da from g = dL/dz and z = the forward OUTPUT (read only by kinds 1 and 2); out[j] at columns >= n
// is not meant to be used.
__device__ __forceinline__ void final_act_bwd4(const float (&g)[4], const float (&z)[4], int n, int kind, int lane, float (&out)[4]) {
    float dot = 0.f;
    if (kind == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) if (lane + 64 * j < n) dot += g[j] * z[j];
        dot = wave_sum(dot);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = kind == 1 ? z[j] * (g[j] - dot) : kind == 2 ? g[j] * z[j] * (1.f - z[j]) : g[j];
}

// ---- COP_DISC_HEAD, one wave per row: from this lane's cells x[j] of the row (columns lane + 64 j; any value at columns
// >= K) and weights w[j] of the discriminator's 1-unit output layer to this lane's cells dx[j] = dL/dlogit * w[j] of dX
// BEFORE the ACTBWD epilogue (chain_actbwd, with the caller's y).  In between: logit, D = sigmoid, the adversarial term
// (mode 0: rows >= row_split are fake; B = row_split), and lane 0's writes - the row's loss term to loss_terms[grow], or
// added to *loss_sum where there is no such buffer, and dL/dlogit to aux_ptr[grow * aux_ld] where the caller keeps it.
// live == false (a row beyond the batch): the wave takes part in the sum and gets dx = 0.
__device__ __forceinline__ void disc_head_row(const float (&x)[4], const float (&w)[4], int K, int lane, bool live, int grow,
                                              int mode, int row_split, float scale, float* loss_terms, float* loss_sum,
                                              float* aux_ptr, int aux_ld, float (&dx)[4]) {
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) if (lane + 64 * j < K) part += x[j] * w[j];
    const float logit = wave_sum(part);
    float gv = 0.f;
    if (live) {
        const float invB = 1.f / (float)row_split;
        const AdvTerm t = adv_term(sigmoidf_(logit), mode == 0 && grow >= row_split, invB, scale);
        gv = t.gv;
        if (lane == 0) {
            if (loss_terms) loss_terms[grow] = -t.l * invB;      // (summed by the weight-gradient launch behind the program)
            else atomicAdd(loss_sum, -t.l * invB);
            if (aux_ptr) aux_ptr[(size_t)grow * aux_ld] = gv;
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) dx[j] = gv * w[j];
}

}  // namespace aae
