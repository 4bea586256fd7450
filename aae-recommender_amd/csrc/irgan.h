// IRGAN (the reference's irgan/cf_gan.py, gen_model.py, dis_model.py): two matrix-factorisation nets G and D, each
//   user_emb [users][dim], item_emb [items][dim], item_bias [items]      fp32, with one momentum buffer each,
// trained by momentum SGD whose gradient is DENSE: every element of all three tensors moves on every step (buf = momentum * buf
// + grad, p -= lr * buf, grad = 0 where the step touches nothing).  All of it is memory- and latency-bound; dim is 5 in the
// reference (rows of 20 bytes), so the vocabulary-sized kernels move item_emb with lanes over CONSECUTIVE FLOATS of a tile of
// kIrTile items (one contiguous block of kIrTile * dim floats) into LDS at the odd row stride dim | 1 and compute from there.
//
//   logit(u, j) = fmaf chain over d = 0 .. dim - 1 starting from item_bias[j]:  acc = fmaf(user_emb[u][d], item_emb[j][d], acc)
//
// SOFTMAX TABLES of a user (irgan_logits_kernel, one workgroup per item tile t):  x_j = logit * inv_temp,  m_t = max of the
// tile, e_j = expf(x_j - m_t) (fp32, stored), s_t = sum of (double) e_j over the tile (a fixed tree).  A combine by ONE workgroup
// (ir_combine): M = max m_t, W_t = s_t * exp(m_t - M) in fp64, cum_t the inclusive prefix of W in ascending t (two levels: a
// thread's contiguous chunk of tiles, the chunks in ascending order), Z = cum of the last tile.  p_j = (float) ((double) e_j * exp(m_t - M) / Z).
//
// SAMPLER (one definition; aaerec/irgan.py restates it).  key = rng_key(seed, draw, 0) ^ sid * 0xA0761D6478BD642F, sid 16 for
// the negatives of generate_for_d, 17 for the samples of a G step; sample i of user u reads w0 = hash_cell(key, u, 2 i) and
// w1 = hash_cell(key, u, 2 i + 1).
//   from p:      x = (w1 + 0.5) * 2^-32, target = x * Z; the tile is the first t with cum_t > target (binary search), the item
//                the first j of that tile, ascending, at which  cum_(t-1) + sum_(i <= j) (double) e_i * exp(m_t - M)  exceeds
//                target (the tile's last item if none does).  A two-level inverse CDF in fp64: accurate at millions of items,
//                one expf per item and step.
//   negatives:   always from p (of the logits / temperature).
//   G samples:   the mixture pn = 0.8 p + 0.2 uniform(pos) taken literally: w0 < 858993459 (0.2 * 2^32) picks the positive
//                pos[(w1 * |pos|) >> 32] of the user's ascending positives, otherwise from p as above.  pn is NOT renormalised
//                (the reference divides by a sum that is 1 up to rounding).
//
// D STEP (n = 2 L triples of L lines (u, pos, neg): (u, pos, 1), (u, neg, 0)):
//   irgan_d_prep_kernel    per triple: the logit from the parameters as they stand, g_t = (sigmoid - label) / n, its BCE term, and
//                          a COPY of both rows it read (the update below then runs in place).
//   irgan_d_update_kernel  one workgroup per tile of kIrTile rows of user_emb or item_emb (+ item_bias).  Every element's owner adds
//                          g_t * (the other side's copied row) over the triples that name its row, IN LIST ORDER (no atomics),
//                          adds the L2 term 2 lambda p / size, and applies the momentum update.  A tile no triple names skips
//                          the scan (one pass over the ids decides).  It leaves its sum of p^2 (fp64, fixed tree) for the loss.
//   irgan_d_loss_kernel    (only when losses are asked for) mean BCE + lambda (mean u^2 + mean v^2 + mean b^2), fp64, fixed order.
// G STEP for user u, n = 2 |pos| samples:
//   irgan_logits_kernel, then irgan_g_sample_kernel (one workgroup: combine; samples injected or drawn; per sample p_s, pn_s,
//   reward_s = 2 (sigmoid(D logit) - 1/2) p_s / pn_s, c_s = reward_s / n, or 0 under the clamp p_s < 1e-8; R = sum c_s and the loss
//   -sum log(max(p_s, 1e-8)) reward_s / n in fp64, fixed order), then irgan_g_update_kernel: an item's logit gradient is
//   gl_j = p_j R - sum_(s = j) c_s (list order), item_emb / item_bias update in place, the tile's part of the user row's gradient
//   sum_j gl_j item_emb[j][d] (old values, fp64, ascending j) is left for irgan_g_user_kernel, and the user tiles carry the
//   momentum into every row but u.  irgan_g_user_kernel adds the parts in ascending tile order and updates row u.
// Every reduction has one fixed order: two runs give the same bits.  No float atomics, no inline assembly.
// Every index is bounded by users, items, the tile or the list lengths the entry points check; an id outside its table (a line,
// an injected sample) contributes nothing.
#pragma once
#include "device_common.h"

namespace aae {

constexpr int kIrTile = 128;          // items (or users) of a workgroup's tile; threads of every workgroup here
constexpr int kIrDimMax = 64;
constexpr int kIrPosMax = 2048;       // most positives of a user: 4096 samples of a G step
constexpr int kIrBatchMax = 1024;     // most lines of a D batch: 2048 triples
constexpr int kIrLds = kIrTile * (kIrDimMax + 1);
constexpr uint32_t kIrSidNeg = 16, kIrSidG = 17;
constexpr uint32_t kIrMixThreshold = 858993459u;      // floor(0.2 * 2^32)

struct IrNet { float* U; float* V; float* b; float* mU; float* mV; float* mb; int users, items, dim; };
// the tables of one user in the caller's scratch: tm / ts / cum [tiles] doubles, e [tiles * kIrTile] floats
struct IrSlot { double* tm; double* ts; double* cum; float* e; };
__host__ __device__ inline IrSlot ir_slot(char* base, size_t stride, int q, int tiles) {
    char* p = base + stride * (size_t)q;
    IrSlot s; s.tm = reinterpret_cast<double*>(p); s.ts = s.tm + tiles; s.cum = s.ts + tiles;
    s.e = reinterpret_cast<float*>(s.cum + tiles);
    return s;
}

__device__ __forceinline__ uint64_t ir_key(uint64_t seed, uint64_t draw, uint32_t sid) {
    return rng_key(seed, draw, 0) ^ ((uint64_t)sid * 0xA0761D6478BD642Full);
}

// a tile of `n` rows of a [rows][dim] table -> LDS at row stride ld: lanes over consecutive floats
__device__ __forceinline__ void ir_stage(const float* __restrict__ tab, int64_t row0, int n, int dim, int ld, float* s) {
    const float* p = tab + row0 * dim;
    for (int f = threadIdx.x; f < n * dim; f += kIrTile) { const int i = f / dim; s[i * ld + (f - i * dim)] = p[f]; }
}

// sum of v over the workgroup in one fixed tree; red: kIrTile doubles of LDS.  Every thread calls it and gets the sum
__device__ __forceinline__ double ir_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = kIrTile >> 1; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ float ir_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

__global__ __launch_bounds__(kIrTile) void irgan_logits_kernel(IrNet G, const int32_t* __restrict__ users, int q0, float inv_temp,
                                                               char* slots, size_t slot_stride) {
    __shared__ float sv[kIrLds];
    __shared__ float su[kIrDimMax];
    __shared__ double red[kIrTile];
    __shared__ float smax[kIrTile];
    const int tid = threadIdx.x, t = blockIdx.x, tiles = gridDim.x, dim = G.dim, ld = dim | 1;
    const IrSlot S = ir_slot(slots, slot_stride, blockIdx.y, tiles);
    const int u = users[q0 + blockIdx.y];
    const int j0 = t * kIrTile, n = min(kIrTile, G.items - j0);
    const bool ok = u >= 0 && u < G.users;
    if (tid < dim) su[tid] = ok ? G.U[(size_t)u * dim + tid] : 0.f;
    ir_stage(G.V, j0, n, dim, ld, sv);
    __syncthreads();
    float x = -INFINITY;
    if (tid < n) {
        float acc = G.b[j0 + tid];
        for (int d = 0; d < dim; ++d) acc = __builtin_fmaf(su[d], sv[tid * ld + d], acc);
        x = acc * inv_temp;
    }
    smax[tid] = x;
    __syncthreads();
    for (int o = kIrTile >> 1; o > 0; o >>= 1) {
        if (tid < o) smax[tid] = fmaxf(smax[tid], smax[tid + o]);
        __syncthreads();
    }
    const float m = smax[0];
    const float e = tid < n ? expf(x - m) : 0.f;
    S.e[j0 + tid] = e;                                  // (the slot holds tiles * kIrTile floats: the padding is zero)
    const double s = ir_sum((double)e, red);
    if (tid == 0) { S.tm[t] = (double)m; S.ts[t] = s; }
}

// M, cum and Z of a slot by the calling workgroup: sh[0] = M, sh[1] = Z.  ts becomes W.  Every thread calls it
__device__ __forceinline__ void ir_combine(const IrSlot& S, int tiles, double* red, double* sh) {
    double m = -INFINITY;
    for (int t = threadIdx.x; t < tiles; t += kIrTile) m = fmax(m, S.tm[t]);
    __syncthreads();
    red[threadIdx.x] = m;
    __syncthreads();
    for (int o = kIrTile >> 1; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + o]);
        __syncthreads();
    }
    const double M = red[0];
    for (int t = threadIdx.x; t < tiles; t += kIrTile) S.ts[t] = S.ts[t] * exp(S.tm[t] - M);
    __syncthreads();
    // the prefix in two levels, one fixed order: a thread sums its contiguous chunk of tiles, thread 0 adds the chunk sums in
    // ascending order (LDS), every thread then writes the running sums of its chunk from the offset it was handed
    const int chunk = (tiles + kIrTile - 1) / kIrTile, t0 = min(tiles, (int)threadIdx.x * chunk), t1 = min(tiles, t0 + chunk);
    double mine = 0.0;
    for (int t = t0; t < t1; ++t) mine += S.ts[t];
    __syncthreads();
    red[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        double acc = 0.0;
        for (int i = 0; i < kIrTile; ++i) { const double v = red[i]; red[i] = acc; acc += v; }
        sh[0] = M;
    }
    __syncthreads();
    double acc = red[threadIdx.x];
    for (int t = t0; t < t1; ++t) { acc += S.ts[t]; S.cum[t] = acc; }
    if (t0 < t1 && t1 == tiles) sh[1] = acc;                      // Z is cum of the last tile, to the bit
    __syncthreads();
}

// the item of `target` in [0, Z): the two-level inverse CDF of the header
__device__ __forceinline__ int ir_pick(double target, const IrSlot& S, int tiles, double M, int items) {
    int lo = 0, hi = tiles - 1;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (S.cum[mid] > target) hi = mid; else lo = mid + 1; }
    const int t = lo, j0 = t * kIrTile, n = min(kIrTile, items - j0);
    double acc = t ? S.cum[t - 1] : 0.0;
    const double scale = exp(S.tm[t] - M);
    for (int i = 0; i < n; ++i) { acc += (double)S.e[j0 + i] * scale; if (acc > target) return j0 + i; }
    return j0 + n - 1;
}
__device__ __forceinline__ double ir_uniform(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }

// generate_for_d: the negatives of users [q0, q0 + gridDim.x) of the list, written into column 2 of their lines
__global__ __launch_bounds__(kIrTile) void irgan_draw_neg_kernel(IrNet G, const int32_t* __restrict__ users,
                                                                 const int64_t* __restrict__ line_off, int q0, int tiles, uint64_t seed,
                                                                 uint64_t draw, int64_t n_lines, int32_t* __restrict__ lines, char* slots,
                                                                 size_t slot_stride) {
    __shared__ double red[kIrTile];
    __shared__ double sh[2];
    const IrSlot S = ir_slot(slots, slot_stride, blockIdx.x, tiles);
    ir_combine(S, tiles, red, sh);
    const int q = q0 + blockIdx.x, u = users[q];
    int64_t lo = line_off[q], hi = line_off[q + 1];
    if (lo < 0 || hi > n_lines || hi - lo > kIrPosMax) return;          // (the entry point refuses what it can see of that)
    const uint64_t key = ir_key(seed, draw, kIrSidNeg);
    for (int i = threadIdx.x; i < (int)(hi - lo); i += kIrTile)
        lines[(lo + i) * 3 + 2] = ir_pick(ir_uniform(hash_cell(key, (uint32_t)u, 2u * i + 1u)) * sh[1], S, tiles, sh[0], G.items);
}

// ascending ids [lo, hi): is j among them
__device__ __forceinline__ bool ir_member(const int32_t* ids, int64_t lo, int64_t hi, int j) {
    int64_t a = lo, b = hi;
    while (a < b) { const int64_t mid = (a + b) >> 1; if (ids[mid] < j) a = mid + 1; else b = mid; }
    return a < hi && ids[a] == j;
}

struct IrGStep {
    const int32_t* users; int step;                       // the step's user: users[step]
    const int64_t* pos_indptr; const int32_t* pos_items;  // ascending positives by user id
    const int32_t* samples; const int64_t* sample_off;    // injected samples (NULL: drawn) and their offsets by step
    uint64_t seed, draw;
    double* hdr;                                          // [0] M  [1] Z  [2] R  [3] n
    int32_t* smp; float* coef;                            // [2 kIrPosMax]
    int32_t* smp_out;                                     // the samples of every step at sample_off (NULL: not wanted)
    double* loss_out;                                     // this step's (NULL: none)
};

__global__ __launch_bounds__(kIrTile) void irgan_g_sample_kernel(IrNet G, IrNet D, IrGStep A, int tiles, char* slots) {
    __shared__ double red[kIrTile];
    __shared__ double sh[2];
    const IrSlot S = ir_slot(slots, 0, 0, tiles);
    ir_combine(S, tiles, red, sh);
    const double M = sh[0], Z = sh[1];
    const int u = A.users[A.step];
    const bool ok = u >= 0 && u < G.users;
    const int64_t plo = ok ? A.pos_indptr[u] : 0, phi = ok ? A.pos_indptr[u + 1] : 0;
    const int npos = (int)(phi - plo) > kIrPosMax ? 0 : (int)(phi - plo);
    const int n = 2 * npos;
    const uint64_t key = ir_key(A.seed, A.draw, kIrSidG);
    double rsum = 0.0, lsum = 0.0;
    for (int i = threadIdx.x; i < n; i += kIrTile) {
        int s;
        if (A.samples) s = A.samples[A.sample_off[A.step] + i];
        else {
            const uint32_t w0 = hash_cell(key, (uint32_t)u, 2u * i), w1 = hash_cell(key, (uint32_t)u, 2u * i + 1u);
            s = w0 < kIrMixThreshold ? A.pos_items[plo + (int64_t)(((uint64_t)w1 * (uint64_t)npos) >> 32)]
                                     : ir_pick(ir_uniform(w1) * Z, S, tiles, M, G.items);
        }
        float c = 0.f;
        if (s >= 0 && s < G.items) {
            const float p = (float)((double)S.e[s] * exp(S.tm[s / kIrTile] - M) / Z);
            const float pn = 0.8f * p + (ir_member(A.pos_items, plo, phi, s) ? 0.2f / (float)npos : 0.f);
            float dl = D.b[s];
            for (int d = 0; d < D.dim; ++d) dl = __builtin_fmaf(D.U[(size_t)u * D.dim + d], D.V[(size_t)s * D.dim + d], dl);
            const float reward = 2.f * (ir_sigmoid(dl) - 0.5f) * p / pn;
            lsum -= (double)(logf(fmaxf(p, 1e-8f)) * reward);
            if (p >= 1e-8f) c = reward / (float)n;
        } else s = -1;
        A.smp[i] = s; A.coef[i] = c;
        if (A.smp_out) A.smp_out[A.sample_off[A.step] + i] = s;
        rsum += (double)c;
    }
    const double R = ir_sum(rsum, red);
    const double L = ir_sum(lsum, red);
    if (threadIdx.x == 0) {
        A.hdr[0] = M; A.hdr[1] = Z; A.hdr[2] = R; A.hdr[3] = (double)n;
        if (A.loss_out) *A.loss_out = n ? L / (double)n : 0.0;
    }
}

// grid: item tiles, then user tiles.  part [tiles][dim] doubles: the tiles' parts of the user row's gradient
__global__ __launch_bounds__(kIrTile) void irgan_g_update_kernel(IrNet G, IrGStep A, int tiles, char* slots, double* __restrict__ part,
                                                                 float lr, float momentum) {
    __shared__ float sv[kIrLds];
    __shared__ float su[kIrDimMax];
    __shared__ float sgl[kIrTile];
    const int tid = threadIdx.x, dim = G.dim, ld = dim | 1;
    const int u = A.users[A.step];
    const int n_s = (int)A.hdr[3];
    if (n_s == 0 || u < 0 || u >= G.users) return;          // (a user without positives: no step)
    if ((int)blockIdx.x >= tiles) {                          // a tile of user rows: the momentum carries on, row u is irgan_g_user_kernel's
        const int r0 = ((int)blockIdx.x - tiles) * kIrTile, n = min(kIrTile, G.users - r0);
        for (int f = tid; f < n * dim; f += kIrTile) {
            if (r0 + f / dim == u) continue;
            const size_t a = (size_t)r0 * dim + f;
            const float buf = momentum * G.mU[a];
            G.mU[a] = buf; G.U[a] -= lr * buf;
        }
        return;
    }
    const IrSlot S = ir_slot(slots, 0, 0, tiles);
    const int t = blockIdx.x, j0 = t * kIrTile, n = min(kIrTile, G.items - j0);
    const double M = A.hdr[0], Z = A.hdr[1], R = A.hdr[2];
    if (tid < dim) su[tid] = G.U[(size_t)u * dim + tid];
    ir_stage(G.V, j0, n, dim, ld, sv);
    int hit = 0;
    for (int i = tid; i < n_s; i += kIrTile) { const int s = A.smp[i]; hit |= (s >= j0 && s < j0 + n); }
    hit = __syncthreads_or(hit);
    if (tid < n) {
        const float p = (float)((double)S.e[j0 + tid] * exp(S.tm[t] - M) / Z);
        double gl = (double)p * R;
        if (hit) {
            double c = 0.0;
            for (int i = 0; i < n_s; ++i) if (A.smp[i] == j0 + tid) c += (double)A.coef[i];
            gl -= c;
        }
        sgl[tid] = (float)gl;
    }
    __syncthreads();
    if (tid < dim) {
        double acc = 0.0;
        for (int i = 0; i < n; ++i) acc += (double)sgl[i] * (double)sv[i * ld + tid];
        part[(size_t)t * dim + tid] = acc;
    }
    for (int f = tid; f < n * dim; f += kIrTile) {
        const int i = f / dim, d = f - i * dim;
        const size_t a = (size_t)j0 * dim + f;
        const float buf = momentum * G.mV[a] + sgl[i] * su[d];
        G.mV[a] = buf; G.V[a] = sv[i * ld + d] - lr * buf;
    }
    if (tid < n) {
        const float buf = momentum * G.mb[j0 + tid] + sgl[tid];
        G.mb[j0 + tid] = buf; G.b[j0 + tid] -= lr * buf;
    }
}

// one workgroup of kIrUserParts x kIrDimMax threads: thread (q, d) adds the tiles of chunk q in ascending order, thread (0, d)
// the chunks in ascending order - one fixed order
constexpr int kIrUserParts = 16;
__global__ __launch_bounds__(kIrUserParts * kIrDimMax) void irgan_g_user_kernel(IrNet G, IrGStep A, int tiles, const double* __restrict__ part,
                                                                                float lr, float momentum) {
    __shared__ double sp[kIrUserParts][kIrDimMax];
    const int d = threadIdx.x % kIrDimMax, q = threadIdx.x / kIrDimMax, u = A.users[A.step];
    if ((int)A.hdr[3] == 0 || u < 0 || u >= G.users) return;          // (the whole workgroup)
    const int chunk = (tiles + kIrUserParts - 1) / kIrUserParts, t0 = min(tiles, q * chunk), t1 = min(tiles, t0 + chunk);
    double acc = 0.0;
    if (d < G.dim) for (int t = t0; t < t1; ++t) acc += part[(size_t)t * G.dim + d];
    sp[q][d] = acc;
    __syncthreads();
    if (q != 0 || d >= G.dim) return;
    acc = 0.0;
    for (int i = 0; i < kIrUserParts; ++i) acc += sp[i][d];
    const size_t a = (size_t)u * G.dim + d;
    const float buf = momentum * G.mU[a] + (float)acc;
    G.mU[a] = buf; G.U[a] -= lr * buf;
}

// ---- D ---------------------------------------------------------------------------------------------------------------------
struct IrDScratch { int32_t* tu; int32_t* ti; float* g; float* bce; float* ru; float* rv; double* l2; };

__global__ __launch_bounds__(kIrTile) void irgan_d_prep_kernel(IrNet D, const int32_t* __restrict__ lines, int n_lines, IrDScratch W) {
    const int t = blockIdx.x * kIrTile + threadIdx.x, n = 2 * n_lines, dim = D.dim;
    if (t >= n) return;
    const int l = t >> 1, u = lines[3 * l], it = lines[3 * l + 1 + (t & 1)];
    const float y = (t & 1) ? 0.f : 1.f;
    const bool ok = u >= 0 && u < D.users && it >= 0 && it < D.items;
    W.tu[t] = ok ? u : -1; W.ti[t] = ok ? it : -1;
    float g = 0.f, bce = 0.f;
    if (ok) {
        float x = D.b[it];
        for (int d = 0; d < dim; ++d) {
            const float a = D.U[(size_t)u * dim + d], b = D.V[(size_t)it * dim + d];
            W.ru[(size_t)t * dim + d] = a; W.rv[(size_t)t * dim + d] = b;
            x = __builtin_fmaf(a, b, x);
        }
        g = (ir_sigmoid(x) - y) / (float)n;
        bce = fmaxf(x, 0.f) - x * y + log1pf(expf(-fabsf(x)));
    }
    W.g[t] = g; W.bce[t] = bce;
}

// grid: user tiles [0, utiles), then item tiles.  l2: [utiles] user parts, [tiles] item parts, [tiles] bias parts
__global__ __launch_bounds__(kIrTile) void irgan_d_update_kernel(IrNet D, int n_triples, IrDScratch W, int utiles, int tiles, float lr,
                                                                 float momentum, float reg_u, float reg_v, float reg_b) {
    __shared__ int sid[2 * kIrBatchMax];
    __shared__ float sg[2 * kIrBatchMax];
    __shared__ double red[kIrTile];
    const int tid = threadIdx.x, dim = D.dim;
    const bool item = (int)blockIdx.x >= utiles;
    const int r0 = (item ? (int)blockIdx.x - utiles : (int)blockIdx.x) * kIrTile;
    const int n = min(kIrTile, (item ? D.items : D.users) - r0);
    const int32_t* ids = item ? W.ti : W.tu;
    const float* other = item ? W.ru : W.rv;              // an item row's gradient reads the user rows, and the reverse
    int hit = 0;
    for (int t = tid; t < n_triples; t += kIrTile) {
        const int id = ids[t];
        sid[t] = id; sg[t] = W.g[t];
        hit |= (id >= r0 && id < r0 + n);
    }
    hit = __syncthreads_or(hit);
    float* P = item ? D.V : D.U;
    float* Mo = item ? D.mV : D.mU;
    const float reg = item ? reg_v : reg_u;
    double sq = 0.0;
    for (int f = tid; f < n * dim; f += kIrTile) {
        const int i = f / dim, d = f - i * dim, row = r0 + i;
        const size_t a = (size_t)r0 * dim + f;
        const float p = P[a];
        float grad = 0.f;
        if (hit) for (int t = 0; t < n_triples; ++t) if (sid[t] == row) grad = __builtin_fmaf(sg[t], other[(size_t)t * dim + d], grad);
        grad += reg * p;
        const float buf = momentum * Mo[a] + grad;
        Mo[a] = buf; P[a] = p - lr * buf;
        sq += (double)p * (double)p;
    }
    const double s1 = ir_sum(sq, red);
    if (tid == 0) W.l2[blockIdx.x] = s1;
    if (!item) return;
    sq = 0.0;
    if (tid < n) {
        const int row = r0 + tid;
        const float p = D.b[row];
        float grad = 0.f;
        if (hit) for (int t = 0; t < n_triples; ++t) if (sid[t] == row) grad += sg[t];
        grad += reg_b * p;
        const float buf = momentum * D.mb[row] + grad;
        D.mb[row] = buf; D.b[row] = p - lr * buf;
        sq = (double)p * (double)p;
    }
    const double s2 = ir_sum(sq, red);
    if (tid == 0) W.l2[blockIdx.x + tiles] = s2;
}

__global__ __launch_bounds__(kIrTile) void irgan_d_loss_kernel(IrNet D, int n_triples, IrDScratch W, int utiles, int tiles, double lambda,
                                                               double* __restrict__ loss_out) {
    __shared__ double red[kIrTile];
    double v = 0.0;
    for (int t = threadIdx.x; t < n_triples; t += kIrTile) v += (double)W.bce[t];
    const double bce = ir_sum(v, red);
    double parts[3];
    const int lo[4] = {0, utiles, utiles + tiles, utiles + 2 * tiles};
    for (int k = 0; k < 3; ++k) {
        v = 0.0;
        for (int t = lo[k] + threadIdx.x; t < lo[k + 1]; t += kIrTile) v += W.l2[t];
        parts[k] = ir_sum(v, red);
    }
    if (threadIdx.x == 0)
        *loss_out = bce / (double)n_triples + lambda * (parts[0] / ((double)D.users * D.dim) + parts[1] / ((double)D.items * D.dim) +
                                                        parts[2] / (double)D.items);
}

// ---- scores ------------------------------------------------------------------------------------------------------------------
// out[r][j] = logit(users[r], j), 0 where j is a training positive of that user (pos_indptr NULL: none); a user id outside the
// table gives a row of zeros.  grid (item tiles, rows strided over grid.y)
__global__ __launch_bounds__(kIrTile) void irgan_scores_kernel(IrNet G, const int32_t* __restrict__ users, int n_rows,
                                                               const int64_t* __restrict__ pos_indptr, const int32_t* __restrict__ pos_items,
                                                               float* __restrict__ out, long long ldo) {
    __shared__ float sv[kIrLds];
    __shared__ float su[kIrDimMax];
    const int tid = threadIdx.x, dim = G.dim, ld = dim | 1;
    const int j0 = blockIdx.x * kIrTile, n = min(kIrTile, G.items - j0);
    ir_stage(G.V, j0, n, dim, ld, sv);
    const float bias = tid < n ? G.b[j0 + tid] : 0.f;
    for (int r = blockIdx.y; r < n_rows; r += gridDim.y) {
        const int u = users[r];
        const bool ok = u >= 0 && u < G.users;
        __syncthreads();                                 // (the tile is staged; the row before this one has been read)
        if (tid < dim) su[tid] = ok ? G.U[(size_t)u * dim + tid] : 0.f;
        __syncthreads();
        if (tid >= n) continue;
        float acc = bias;
        for (int d = 0; d < dim; ++d) acc = __builtin_fmaf(su[d], sv[tid * ld + d], acc);
        if (!ok || (pos_indptr && ir_member(pos_items, pos_indptr[u], pos_indptr[u + 1], j0 + tid))) acc = 0.f;
        out[(size_t)r * ldo + j0 + tid] = acc;
    }
}

}  // namespace aae
